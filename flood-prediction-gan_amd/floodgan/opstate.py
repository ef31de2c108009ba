"""Operand-scale state of a tensor: one versioned record, stored on the tensor object as `t._fg`.

Which absmax slot bounds a tensor (the f16x3 math's scale source), which format its storage holds and the split
copy made from it are facts about the tensor's CONTENTS, so they carry one stamp, torch's version counter when they
were recorded: a record is current iff state.version == t._version.  The kernels write through raw pointers (the
counter does not move), so every op that writes a tensor calls wrote(t), and a producer that raises a slot over
what it wrote calls record_slot, the only place that stamps a version.  An in-place torch write moves the counter
(views share their base's) and so invalidates slot, format and split copy at once; a stale record of a non-fp32
format is an error where it is read (current), never a silent fall back to fp32.  Weight packs stand apart from the
stamp: a pack is current while the slot it was scaled by (pack_slot) is the parameter's current slot.
Imports only torch, so a CPU test can hold the invariant.
"""
import torch

FP32, PRESPLIT, SPLITPIX = 0, 1, 2      # the storage holds fp32 values / FG_PRESPLIT pieces / fg_split_pixels' layout

_STALE = {PRESPLIT: "a pre-split (FG_PRESPLIT) buffer was written by torch since its producer ran",
          SPLITPIX: "a split-pixels buffer was written by torch since its producer ran"}


class OperandState:
    __slots__ = ("version", "slot", "fmt", "split", "packs")

    def __init__(self):
        self.version = None     # t._version when slot, fmt and split were recorded
        self.slot = None        # the absmax slot tensor
        self.fmt = FP32
        self.split = None       # (fg_split_pixels copy, the slot it was scaled by)
        self.packs = None       # parameters: {bytes(fg_weight_map): (packed tensor, map struct)}


def tensor(obj):
    """tensor | Buf | Slice (a Slice maps to its buffer's tensor) -> the tensor that carries the record"""
    return obj if isinstance(obj, torch.Tensor) else obj.t


def current(obj):
    """the record of obj if it is current, else None; a stale record of a non-fp32 format raises"""
    t = tensor(obj)
    st = t.__dict__.get("_fg")
    if st is None or st.version == t._version:
        return st
    if st.fmt != FP32:
        raise RuntimeError(_STALE[st.fmt])
    return None


def wrote(*objs):
    """an op wrote these (None | tensor | Buf | Slice): drop slot, split copy and format, keep packs; creates none"""
    for o in objs:
        if o is not None:
            st = tensor(o).__dict__.get("_fg")
            if st is not None:
                st.slot, st.split, st.fmt = None, None, FP32


def record_slot(obj, slot, fmt=FP32, split=None):
    """a producer raised `slot` over obj's contents (of format fmt; split: their (copy, slot)): stamp obj's version"""
    t = tensor(obj)
    st = t.__dict__.get("_fg")
    if st is None:
        st = t._fg = OperandState()
    st.version, st.slot, st.fmt, st.split = t._version, slot, fmt, split


def adopt(dst, src):
    """dst, a view of src's storage, takes src's current slot (it bounds the whole storage) and format, if any"""
    st = current(src)
    if st is not None and st.slot is not None:
        assert st.fmt != SPLITPIX, "a view of a split-pixels buffer has no split layout of its own"
        record_slot(dst, st.slot, st.fmt)


def keep_slot_across(obj):
    """an in-place write that cannot grow |obj| is about to run: the current slot (returned, or None) still
    bounds the contents and stays; the split copy and the format are dropped"""
    t = tensor(obj)
    st = t.__dict__.get("_fg")
    if st is None:
        return None
    if st.version != t._version:
        st.slot = None
    st.split, st.fmt = None, FP32
    return st.slot


def slot_of(obj):
    """the current absmax slot of obj, or None"""
    st = current(obj)
    return None if st is None else st.slot


def is_presplit(obj):
    st = current(obj)
    return st is not None and st.fmt == PRESPLIT


def is_splitpix(obj):
    st = current(obj)
    return st is not None and st.fmt == SPLITPIX


def packs(w):
    """the pack cache of a parameter that has a record (absmax(w) made one), else None"""
    st = w.__dict__.get("_fg")
    if st is not None and st.packs is None:
        st.packs = {}
    return None if st is None else st.packs


def pack_slot(wp):
    """the absmax slot a packed weight tensor was scaled by (its packer's record_slot(wp, slot)), or None"""
    st = wp.__dict__.get("_fg")
    return None if st is None else st.slot
