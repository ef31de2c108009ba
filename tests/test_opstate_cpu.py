"""The operand-scale record (floodgan/opstate.py) on CPU tensors: torch's version counter and attribute behaviour
are the same as on the device.  One rule is held here: slot, format and split copy are current iff the record's
version equals the tensor's."""
import pytest
import torch

from floodgan import opstate as S
from floodgan.plans import Buf, Slice


def _slot():
    return torch.zeros(64)


def test_recorded_slot_is_current_until_a_torch_write():
    t, slot = torch.ones(8), _slot()
    assert S.current(t) is None and S.slot_of(t) is None
    S.record_slot(t, slot)
    st = S.current(t)
    assert st is t._fg and st.version == t._version and st.slot is slot and st.fmt == S.FP32 and st.split is None
    assert S.slot_of(t) is slot and not S.is_presplit(t) and not S.is_splitpix(t)
    t.add_(1)
    assert S.current(t) is None and S.slot_of(t) is None          # an fp32 record goes stale without raising
    assert not S.is_presplit(t) and not S.is_splitpix(t)


@pytest.mark.parametrize("fmt, reader, text", [
    (S.PRESPLIT, S.is_presplit, "a pre-split (FG_PRESPLIT) buffer was written by torch since its producer ran"),
    (S.SPLITPIX, S.is_splitpix, "a split-pixels buffer was written by torch since its producer ran")])
def test_stale_non_fp32_record_raises(fmt, reader, text):
    t = torch.ones(8)
    S.record_slot(t, _slot(), fmt)
    assert reader(t)
    t.mul_(2)
    for read in (reader, S.current, S.slot_of, S.is_presplit, S.is_splitpix):
        with pytest.raises(RuntimeError) as e:
            read(t)
        assert str(e.value) == text
    S.wrote(t)                                  # the producer that overwrites it next does not raise
    assert S.current(t) is None
    S.record_slot(t, _slot())
    assert S.slot_of(t) is not None and not reader(t)


def test_wrote_clears_slot_split_format_and_keeps_packs():
    w, slot = torch.ones(8), _slot()
    S.record_slot(w, slot, S.PRESPLIT, split=(torch.zeros(16, dtype=torch.float16), slot))
    packs = S.packs(w)
    packs[b"map"] = (torch.zeros(4), object())
    S.wrote(w)
    st = w._fg
    assert st.slot is None and st.split is None and st.fmt == S.FP32
    assert S.slot_of(w) is None and not S.is_presplit(w)
    assert S.packs(w) is packs and list(packs) == [b"map"]
    S.record_slot(w, _slot())                   # nor does a new slot drop them
    assert S.packs(w) is packs and list(packs) == [b"map"]


def test_wrote_never_creates_a_record_and_takes_none_buf_slice():
    t = torch.ones(8)
    S.wrote(t)
    S.wrote(None, t, None)
    assert not hasattr(t, "_fg") and S.packs(t) is None and S.pack_slot(t) is None
    buf = Buf(torch.ones(2 * 3 * 3 * 8), 2, 3, 3, 8)
    S.wrote(buf, Slice(buf, 4, 4))
    assert not hasattr(buf.t, "_fg")
    for writer in (buf, Slice(buf, 0, 4)):      # a Slice maps to its buffer's tensor
        slot = _slot()
        S.record_slot(buf, slot, S.PRESPLIT)
        assert S.slot_of(Slice(buf, 4, 4)) is slot and S.is_presplit(Slice(buf, 4, 4)) and S.slot_of(buf.t) is slot
        S.wrote(None, writer)
        assert S.slot_of(buf) is None and not S.is_presplit(buf)


@pytest.mark.parametrize("fmt", [S.FP32, S.PRESPLIT])
@pytest.mark.parametrize("through", ["base", "view"])
def test_adopt_on_a_slice_view(fmt, through):
    t, slot = torch.ones(12), _slot()
    v = t[4:8]
    S.adopt(v, t)
    assert not hasattr(v, "_fg")                # nothing to adopt yet
    S.record_slot(t, slot, fmt)
    S.adopt(v, t)
    st = S.current(v)
    assert st is not None and st is not t._fg and st.version == v._version
    assert st.slot is slot and S.slot_of(v) is slot and st.fmt == fmt and S.is_presplit(v) == (fmt == S.PRESPLIT)
    assert v._version == t._version
    (t if through == "base" else v).add_(1)
    assert v._version == t._version             # torch shares the counter between a view and its base
    for x in (t, v):
        if fmt == S.FP32:
            assert S.current(x) is None and S.slot_of(x) is None
        else:
            with pytest.raises(RuntimeError):
                S.current(x)


def test_adopt_ignores_a_stale_source():
    t = torch.ones(12)
    S.record_slot(t, _slot())
    t.add_(1)
    v = t[:4]
    S.adopt(v, t)
    assert not hasattr(v, "_fg")


def test_keep_slot_across_keeps_the_slot_and_drops_split_and_format():
    t, slot = torch.ones(8), _slot()
    assert S.keep_slot_across(t) is None and not hasattr(t, "_fg")
    S.record_slot(t, slot, S.PRESPLIT, split=(torch.zeros(16, dtype=torch.float16), slot))
    assert S.keep_slot_across(t) is slot
    st = S.current(t)
    assert st.slot is slot and S.slot_of(t) is slot and st.split is None and st.fmt == S.FP32
    t.add_(1)                                   # a stale slot is not kept
    assert S.keep_slot_across(t) is None and t._fg.slot is None and S.slot_of(t) is None


def test_format_is_exclusive():
    t = torch.ones(8)
    S.record_slot(t, _slot(), S.PRESPLIT)
    assert S.is_presplit(t) and not S.is_splitpix(t)
    slot = _slot()
    S.record_slot(t, slot, S.SPLITPIX, split=(t.view(torch.float16), slot))
    assert S.is_splitpix(t) and not S.is_presplit(t) and S.current(t).fmt == S.SPLITPIX
    S.record_slot(t, _slot())
    assert not S.is_splitpix(t) and not S.is_presplit(t) and S.current(t).split is None


def test_pack_slot_reads_the_packers_record():
    wp, slot = torch.zeros(8, dtype=torch.float16), _slot()
    assert S.pack_slot(wp) is None
    S.record_slot(wp, slot)
    assert S.pack_slot(wp) is slot
