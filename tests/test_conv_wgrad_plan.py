"""The weight gradient's planning rule (conv_mfma.hip plan_wgrad, read through
scae_conv3x3_wgrad_tile_plan) at the encoder layers of bench.py's four workloads, and the split
counts it must leave alone.  Host functions only: no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# workload -> the split count of its layers 2, 3, 4 (what the library returned before the tile
# forms existed: the partial-slab layout depends on it)
SPLITS = {"mnist_24_24_bs128": [22, 22, 12], "mnist_40_32_bs128": [22, 22, 12],
          "mnist_48_64_bs1024": [22, 22, 22], "cifar_32_32_bs256": [22, 22, 9]}


@pytest.mark.parametrize("workload", sorted(SPLITS))
def test_the_planned_tile_and_the_splits_of_a_workloads_encoder_layers(workload):
    import bench
    from torch_scae_amd import _lib
    lib, cfg = _lib.load(), bench.CONFIGS[workload]
    layers = bench.conv_layers(cfg)
    assert [(ci, co) for _, ci, co, _ in layers] == [(128, 128)] * 3
    lead_128x64 = _lib.WGRAD_TILE_128x64 | _lib.WGRAD_HEAD
    assert lead_128x64 == 66
    got_splits, got_tiles = [], []
    for IH, Ci, Co, s in layers:
        OH = (IH - 3) // s + 1
        got_splits.append(lib.scae_conv3x3_wgrad_splits(cfg["batch"], OH, OH, Ci, Co))
        got_tiles.append(lib.scae_conv3x3_wgrad_tile_plan(cfg["batch"], IH, IH, Ci, Co, s,
                                                          _lib.DGRAD_BY_SHAPE))
    assert got_splits == SPLITS[workload]
    # every one of these layers runs beside DMA-fed data-gradient tiles on 32-pixel chunks
    assert got_tiles == [lead_128x64] * 3


def test_the_rule_away_from_the_measured_layers():
    from torch_scae_amd import _lib
    lib = _lib.load()
    plain = _lib.WGRAD_TILE_64x64
    # first-generation data-gradient tiles: as before
    assert lib.scae_conv3x3_wgrad_tile_plan(128, 19, 19, 128, 128, 2,
                                            _lib.DGRAD_NO_TILE | _lib.DGRAD_NO_KSPLIT) == plain
    # a short layer beside the DMA-fed tile (16-pixel quantum): as before
    assert lib.scae_conv3x3_wgrad_tile_plan(30, 9, 9, 128, 128, 1, _lib.DGRAD_TILE) == plain
    # output channels 128 does not divide: the 64 x 64 tiles lead
    assert lib.scae_conv3x3_wgrad_tile_plan(128, 19, 19, 128, 64, 2, 0) == plain | _lib.WGRAD_HEAD
    # rejected arguments
    assert lib.scae_conv3x3_wgrad_tile_plan(128, 19, 19, 128, 128, 2, 8) == _lib.ERR_BAD_ARG
    assert lib.scae_conv3x3_wgrad_tile_plan(128, 19, 19, 128, 128, 0, 0) == _lib.ERR_BAD_ARG
    assert lib.scae_conv3x3_wgrad_tile_plan(128, 19, 19, 100, 128, 2, 0) == _lib.ERR_UNSUPPORTED
