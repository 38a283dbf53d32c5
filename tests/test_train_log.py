"""CPU checks of the training log's host side (TrainStep(log_steps=N)): the ring's unrolling
order, the argument checks, and the key <-> row map against include/scae_hip.h."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "scae_hip.h")).read()


def test_ring_order_unrolls_oldest_first_and_wraps():
    from torch_scae_amd.ops import ring_order
    assert ring_order(0, 4) == ([], [])
    assert ring_order(3, 4) == ([0, 1, 2], [0, 1, 2])
    assert ring_order(4, 4) == ([0, 1, 2, 3], [0, 1, 2, 3])
    assert ring_order(10, 4) == ([2, 3, 0, 1], [6, 7, 8, 9])
    assert ring_order(5, 1) == ([0], [4])
    assert ring_order(8, 4) == ([0, 1, 2, 3], [4, 5, 6, 7])


def _cpu_model():
    from torch_scae_amd import factory
    cfg = dict(image_shape=(1, 16, 16), n_classes=4, n_part_caps=5, n_obj_caps=4,
               pcae_cnn_encoder_params=dict(out_channels=[8, 8], kernel_sizes=[3, 3],
                                            strides=[2, 1]),
               pcae_template_generator_params=dict(template_size=(5, 5)),
               ocae_encoder_set_transformer_params=dict(dim_hidden=8, dim_out=8, n_layers=1),
               ocae_decoder_capsule_params=dict(dim_caps=4, hidden_sizes=(8,)),
               scae_params=dict(reconstruct_alternatives=False))
    torch.manual_seed(0)
    return factory.make_scae(cfg)


@pytest.mark.parametrize("bad", [-1, 2.5, True, "8"])
def test_log_steps_must_be_a_non_negative_int(bad):
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError, match="log_steps"):
        TrainStep(_cpu_model(), 4, (1, 16, 16), log_steps=bad)


def test_log_steps_needs_a_hip_device():
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError, match="HIP device"):
        TrainStep(_cpu_model(), 4, (1, 16, 16), log_steps=8)


def test_row_map_agrees_with_the_header_and_the_accumulator():
    from torch_scae_amd import _lib
    from torch_scae_amd.eval_step import ACC_KEYS
    from torch_scae_amd.ops import TRAIN_LOG_INDEX
    h = _header()
    row = int(re.search(r"#define SCAE_TRAIN_LOG_ROW (\d+)", h).group(1))
    assert row == _lib.TRAIN_LOG_ROW
    idx = sorted(TRAIN_LOG_INDEX.values())
    # every entry has one key, but [4]: the 12-vector's loss, the same value as [0]
    assert idx == [i for i in range(row) if i != 4]
    # the accumulator's keys sit one place earlier in the row ([0] counts batches there)
    for k, i in ACC_KEYS.items():
        assert TRAIN_LOG_INDEX[k] == i - 1, k
    # the row's documented layout
    assert "[16] learning rate" in h and "[4 + i] out12[i]" in h
    assert TRAIN_LOG_INDEX["learning_rate"] == 16
    assert TRAIN_LOG_INDEX["mse"] == 17 and TRAIN_LOG_INDEX["part_caps_loss"] == 18


def _struct_fields(h, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s*]", "", n).split()[-1] if n.strip() else n
                      for n in re.sub(r"^.*?\b(?:float|int|int64_t|double|"
                                      r"scae_train_log_desc)\b\s*", "", decl).split(",")]
    return [n.strip("*").strip() for n in names]


def test_descriptor_and_extras_mirror_the_header():
    from torch_scae_amd import _lib
    h = _header()
    assert _struct_fields(h, "scae_train_log_desc") == \
        [f for f, _ in _lib.TrainLogDesc._fields_]
    extras = _struct_fields(h, "scae_loss_extras")
    assert extras == [f for f, _ in _lib.LossExtras._fields_]
    assert extras[-1] == "train_log"        # (appended: the earlier fields keep their place)
