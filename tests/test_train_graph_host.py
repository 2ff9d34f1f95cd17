"""Host side of graph.TrainStep, no GPU needed: the fixed-shape target packing, the byte layout of the step-scalar record
the `_dev` updates read from device memory, the counter helpers that fill it, and the header's declarations."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vrnet_mt_sgd_dev_f32", "vrnet_mt_adam_dev_f32", "vrnet_mt_ema_dev_f32", "vrnet_adam_bias_correction")


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    import asy_vrnet_amd.hip as hip
    return hip


def test_pack_targets_layout(hip):
    from asy_vrnet_amd import losses
    rows = [torch.arange(10, dtype=torch.float64).reshape(2, 5), None, torch.zeros((0, 5)), torch.full((3, 5), 7.5)]
    packed, counts = losses.pack_targets(rows, 3)
    assert packed.dtype == torch.float32 and tuple(packed.shape) == (4, 3, 5) and not packed.is_cuda
    assert counts.dtype == torch.int32 and counts.tolist() == [2, 0, 0, 3]
    want = torch.zeros(4, 3, 5)
    want[0, :2] = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    want[3] = 7.5
    assert torch.equal(packed, want)
    # in place, over stale contents
    out, cnt = torch.full((4, 3, 5), -1.0), torch.full((4,), -1, dtype=torch.int32)
    got = losses.pack_targets(rows, 3, out=out, counts_out=cnt)
    assert got[0] is out and got[1] is cnt and torch.equal(out, want) and cnt.tolist() == [2, 0, 0, 3]


def test_pack_targets_errors_name_the_image_and_write_nothing(hip):
    from asy_vrnet_amd import losses
    out, cnt = torch.full((3, 2, 5), -1.0), torch.full((3,), -1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="image 2"):
        losses.pack_targets([torch.ones(1, 5), None, torch.ones(3, 5)], 2, out=out, counts_out=cnt)
    assert (out == -1).all() and (cnt == -1).all()
    with pytest.raises(RuntimeError, match="image 0"):
        losses.pack_targets([torch.ones(2, 4)], 2)
    with pytest.raises(RuntimeError, match="buffers"):
        losses.pack_targets([torch.ones(1, 5)], 2, out=torch.zeros(1, 3, 5))


def test_step_scalar_record_layout(hip):
    dt = np.dtype([("lr", "<f4"), ("ema_decay", "<f4"), ("adam_bc1", "<f4"), ("adam_bc2_sqrt", "<f4")])
    assert ctypes.sizeof(hip.StepScalars) == 16 == dt.itemsize
    assert [(n, getattr(hip.StepScalars, n).offset) for n, _ in hip.StepScalars._fields_] == \
        [(n, dt.fields[n][1]) for n in dt.names]
    rec = hip.StepScalars(0.01, 0.63, 0.1, 0.03)
    got = np.frombuffer(bytes(rec), dtype=dt)[0]
    assert [got[n] for n in dt.names] == [np.float32(v) for v in (0.01, 0.63, 0.1, 0.03)]
    # the header's struct: four floats in this order
    text = open(os.path.join(ROOT, "include", "vrnet_hip.h")).read()
    body = re.search(r"typedef struct vrnet_step_scalars \{(.*?)\} vrnet_step_scalars;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"float\s+(\w+)\s*;", body) == list(dt.names)


@pytest.mark.parametrize("n", [1, 2, 2000])
def test_ema_advance_returns_the_float_decay_and_counts(hip, n):
    from asy_vrnet_amd import optim
    decay, tau = 0.9999, 2000
    ema = optim.ModelEMA(torch.nn.Linear(2, 2), decay=decay, tau=tau, updates=n - 1)
    d = ema.advance()
    assert ema.updates == n
    assert d == np.float32(decay * (1 - math.exp(-n / tau)))
    assert np.float32(d) == d            # already a float32 value: the record holds it unchanged


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("b1,b2", [(0.9, 0.999), (0.937, 0.999)])
def test_adam_bias_correction_is_the_double_precision_expression(hip, step, b1, b2):
    bc1, bc2s = hip.adam_bias_correction(b1, b2, step)
    f1, f2 = float(np.float32(b1)), float(np.float32(b2))          # the C-ABI takes the betas as floats
    assert bc1 == np.float32(1.0 - math.pow(f1, step))
    assert bc2s == np.float32(math.sqrt(1.0 - math.pow(f2, step)))
    with pytest.raises(RuntimeError, match="step counts from 1"):
        hip.adam_bias_correction(b1, b2, 0)


def test_header_declares_the_new_symbols(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrnet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vrnet_\w+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(hip.EXPORTED)
    assert all(callable(getattr(hip, n)) for n in ("mt_sgd_dev", "mt_adam_dev", "mt_ema_dev", "adam_bias_correction"))
    from asy_vrnet_amd import graph, losses
    assert callable(graph.TrainStep) and callable(losses.training_loss_packed)
