"""floodgan -- MI355X-native (gfx950) PairedAttention paired-GAN training step and its neighbours.

Drop-in for the reference's hot path (Natasha-R/Flood-Prediction-GAN,
models/model_architectures.py:305-441 + models/model.py:598-658): the module classes and
the Model/train_paired API mirror the reference, the arithmetic runs in hand-written HIP
kernels (libfloodgan.so, C-ABI in include/floodgan.h).  Around it: the cycle models
(train_cycle), the tile data path (floodgan.data), Pix2Pix (U-Net-256 + BatchNorm PatchGAN) and the
evaluation path (segmentation U-Net, device metrics: floodgan.evaluate); torch.library operators in
floodgan.custom_ops; pictures of predictions, attention and flood masks as PNG files
(floodgan.render, floodgan.png: converted and composed on the device, encoded on the host); whole scenes
through a generator in overlapping windows blended on the device (floodgan.scene); the flood regions of a scene --
connected components, minimum-mapping-unit sieve, region table -- on the device (floodgan.regions); the flood depth
of a scene from its mask and elevation -- exact nearest-shore transform, depth plane, per-region depth table -- on the
device (floodgan.depth); the outlines of the regions as polygons, traced on the device, and their GeoJSON file
(floodgan.outline); the drainage of a scene's elevation -- D8 flow directions, flow accumulation, basins and path
lengths -- on the device (floodgan.flow).
"""
from ._lib import load as load_library  # noqa: F401
from .model_architectures import (AttentionGANBlock, AttentionGANDiscriminator,  # noqa: F401
                                  AttentionGANGenerator, CycleGANBlock, CycleGANDiscriminator, CycleGANGenerator,
                                  PairedAttentionBlock, PairedAttentionDiscriminator, PairedAttentionGenerator,
                                  Pix2PixBlock, Pix2PixDiscriminator, Pix2PixGenerator)
from .segmentation import FloodMaskLoss, UNet  # noqa: F401
from .evaluate import LPIPS, compare_output_images, load_lpips_weights  # noqa: F401
from .png import read_png, write_png  # noqa: F401
from .render import Canvas, colormap_lut, save_image, save_sheet, sheet_layout  # noqa: F401
from .scene import Mosaic, predict_scene, window_grid  # noqa: F401
from .regions import flood_regions, label_regions, write_regions_csv  # noqa: F401
from .depth import flood_depth, nearest_seed  # noqa: F401
from .outline import region_outlines, write_regions_geojson  # noqa: F401
from .flow import flow_accumulation, flow_directions, render_flow  # noqa: F401
from .data import load_scene_elevation  # noqa: F401

__all__ = ["PairedAttentionGenerator", "PairedAttentionBlock", "PairedAttentionDiscriminator",
           "AttentionGANGenerator", "AttentionGANBlock", "AttentionGANDiscriminator",
           "CycleGANGenerator", "CycleGANBlock", "CycleGANDiscriminator",
           "Pix2PixGenerator", "Pix2PixBlock", "Pix2PixDiscriminator", "UNet", "FloodMaskLoss", "load_library", "LPIPS",
           "load_lpips_weights", "Canvas", "colormap_lut", "save_image", "save_sheet", "sheet_layout", "write_png",
           "read_png", "compare_output_images", "Mosaic", "predict_scene", "window_grid", "flood_regions",
           "label_regions", "write_regions_csv", "nearest_seed", "flood_depth", "load_scene_elevation",
           "region_outlines", "write_regions_geojson", "flow_directions", "flow_accumulation", "render_flow"]
