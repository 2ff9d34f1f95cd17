"""The C calls the Python layer issues for the inference-side frame ops, pinned: every call of the library that one
`FramePipeline.run`, one `EvalPipeline.add` or one direct call of render / decode makes -- entry point and arguments, in order
-- equals the trace in tests/golden/frame_op_calls.json, which was recorded before the fixed-size and `_ragged` wrappers
of hip.py, render.py and decode.py were folded into one body each.  A pointer argument is recorded as null / non-null, an
integer exactly, a float by repr.  The model's own forward is muted: only the frame ops are traced.

The fixture is written by this module itself, `python -m tests.test_frame_op_calls [path]` from the repository root, on the
commit BEFORE a change to those wrappers; it is never regenerated from the changed tree."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import asy_vrnet_amd as A
from asy_vrnet_amd import data, decode, hip, render
from tests import labels_cases as LC

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_op_calls.json")
NC, NSEG, S, F, B = 4, 9, (64, 64), (48, 64), 2
SIZES = [(48, 64), (37, 53)]                    # of a ragged batch, inside the capacity F
NAMES = ["boat", "buoy", "pier", "ship"]
EVERYTHING = dict(render=True, heatmap=True, crops=True, dehaze=True, normalise_radar=True)
_atlas = {}
_NUMBERS = {hip.I: int, hip.L: int, hip.F: lambda v: repr(float(v)), hip.D: lambda v: repr(float(v))}


class Recorder:
    """Stands in for `hip._lib`: every entry point of `hip._SIGS` called through it is noted, unless `muted`."""

    def __init__(self, lib):
        self._lib, self.calls, self.muted = lib, [], True

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in hip._SIGS:
            return fn
        kinds = [_NUMBERS.get(t) for t in hip._SIGS[name][0]]

        def call(*args):
            if not self.muted:
                assert len(args) == len(kinds), name
                self.calls.append([name, [("null" if not a else "ptr") if k is None else k(a) for k, a in zip(kinds, args)]])
            return fn(*args)
        return call


def atlas():
    """The committed atlas fixture of tests/test_labels.py, never one built by the Pillow at hand: the blob's size is an argument."""
    if "a" not in _atlas:
        _atlas["a"] = render.LabelAtlas.load(LC.FIXTURE)
    return _atlas["a"]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def inputs(seed, sizes):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    radar = (rng.standard_normal((B, 4) + S) * 2.0 + 1.0).astype(np.float32)
    return frames, radar, rng


def geometry(letterbox_image=True):
    table = data.frame_geometry(SIZES, S, letterbox_image, F, data.default_max_taps(F, S), "test")
    return data.geometry_bytes(table).cuda()


def host_results(rng):
    """What `non_max_suppression` returns for a batch of two: three rows, and an image without detections."""
    rows = np.array([[4.2, 6.9, 30.5, 40.1, 0.9, 0.8, 1], [10.0, 20.0, 44.0, 60.0, 0.7, 0.6, 3], [0.0, 0.0, 47.9, 63.9, 0.5, 0.5, 0]],
                    np.float32)
    return [rows, None]


def device_triple(rng):
    cases = [LC.random_case(rng, 37, 53, n, 1) for n in (3, 2)]
    rows, offsets, scores = LC.pack(cases)
    return cuda(rows), cuda(offsets), cuda(LC.label_indices(rows, scores))


def levels(rng):
    return [cuda(rng.standard_normal((B, 5 + NC, S[0] // s, S[1] // s)).astype(np.float32)) for s in (8, 16, 32)]


# ---- the cases: each builds its inputs (not traced) and returns the call that is ----------------------------------------
def frame_pipeline(ragged, **kw):
    def build(model):
        if kw.get("render"):
            kw["labels"] = atlas()
        pipe = A.FramePipeline(model, F, S, batch=B, conf_thres=0.3, nms_thres=0.5, max_candidates=32, graph=False, ragged=ragged, **kw)
        frames, radar, _ = inputs(21, SIZES if ragged else [F] * B)
        return lambda: pipe.run(frames if ragged else np.stack(frames), radar)
    return build


def eval_pipeline(ragged):
    def build(model):
        pipe = A.EvalPipeline(model, F, S, NAMES, NSEG, batch=B, capacity=B, max_boxes=4, max_gt=4, graph=False, ragged=ragged)
        sizes = SIZES if ragged else [F] * B
        frames, radar, rng = inputs(22, sizes)
        labels = [rng.integers(0, NSEG, s).astype(np.uint8) for s in sizes]
        gt = [np.array([[3, 4, 20, 30, 1], [8, 2, 40, 33, 0]], np.int64), np.zeros((0, 5), np.int64)]
        if not ragged:
            frames, labels = np.stack(frames), np.stack(labels)
        return lambda: pipe.add(["a", "b"], frames, radar, labels, gt)
    return build


def render_frame_host(model):
    frames, _, rng = inputs(23, [F] * B)
    cmap, flag = rng.integers(0, NSEG, (B,) + F).astype(np.uint8), new_flag()
    return lambda: render.render_frame(np.stack(frames), cmap, host_results(rng), S, palette=render.seg_palette(NSEG), count=True,
                                       flag=flag, labels=atlas())


def draw_labels_host(model):
    frames, _, rng = inputs(24, [F] * B)
    picture, flag = cuda(np.stack(frames)), new_flag()
    return lambda: render.draw_labels(picture, host_results(rng), atlas(), S, flag=flag)


def heatmap_fixed(letterbox_image, mask_only):
    def build(model):
        frames, _, rng = inputs(25, [F] * B)
        lv = levels(rng)
        if mask_only:
            return lambda: render.heatmap_mask(lv, F, S, letterbox_image)
        return lambda: render.heatmap(np.stack(frames), lv, S, letterbox_image, alpha=0.6)
    return build


def seg_predict_fixed(model):
    seg = cuda(np.random.default_rng(26).standard_normal((B, NSEG) + S).astype(np.float32))
    return lambda: decode.seg_predict(seg, S, F)


def render_frame_ragged(model):
    _, _, rng = inputs(27, SIZES)
    frames, cmap = cuda(rng.integers(0, 256, (B,) + F + (3,), dtype=np.uint8)), cuda(rng.integers(0, NSEG, (B,) + F).astype(np.uint8))
    geom, triple, flag = geometry(), device_triple(rng), new_flag()
    tab = cuda(atlas().size_table([s[0] for s in SIZES]))
    return lambda: render.render_frame_ragged(frames, geom, cmap, triple, palette=render.seg_palette(NSEG), count=True, flag=flag,
                                              labels=atlas(), label_sizes=tab)


def heatmap_ragged(window):
    def build(model):
        _, _, rng = inputs(28, SIZES)
        frames, lv, geom, flag = cuda(rng.integers(0, 256, (B,) + F + (3,), dtype=np.uint8)), levels(rng), geometry(), new_flag()
        return lambda: render.heatmap_ragged(frames, lv, geom, S, window=window, alpha=0.6, flag=flag)
    return build


def seg_predict_ragged(model):
    seg, geom, flag = cuda(np.random.default_rng(29).standard_normal((B, NSEG) + S).astype(np.float32)), geometry(), new_flag()
    return lambda: decode.seg_predict_ragged(seg, geom, F, flag)


CASES = {
    "FramePipeline fixed, everything on": frame_pipeline(False, **EVERYTHING),
    "FramePipeline fixed, plain, letterbox_image=False": frame_pipeline(False, letterbox_image=False),
    "FramePipeline ragged, everything on": frame_pipeline(True, **EVERYTHING),
    "FramePipeline ragged, letterbox_image=False, render=False": frame_pipeline(True, letterbox_image=False, render=False),
    "EvalPipeline fixed": eval_pipeline(False),
    "EvalPipeline ragged": eval_pipeline(True),
    "render.render_frame, host results and labels": render_frame_host,
    "render.draw_labels, host results": draw_labels_host,
    "render.heatmap_mask": heatmap_fixed(False, True),
    "render.heatmap_mask, letterbox_image=True": heatmap_fixed(True, True),
    "render.heatmap": heatmap_fixed(False, False),
    "render.heatmap, letterbox_image=True": heatmap_fixed(True, False),
    "decode.seg_predict": seg_predict_fixed,
    "render.render_frame_ragged, device triple and labels": render_frame_ragged,
    "render.heatmap_ragged": heatmap_ragged(True),
    "render.heatmap_ragged, window=False": heatmap_ragged(False),
    "decode.seg_predict_ragged": seg_predict_ragged,
}


def make_model():
    model = A.EfficientVRNet(NC, NSEG, "nano", img_size=S[0]).cuda().eval()
    A.randomize_state_dict(model.state_dict(), seed=4)
    return model


def trace(name, model, patch):
    """The calls of one case.  The scratch arena of hip.py is grow-only and shared, so its size -- an argument of the
    letterbox calls -- would depend on what ran before: the case gets a fresh one."""
    rec = Recorder(hip._lib)
    patch.setattr(hip, "_ws", hip.Workspace())
    patch.setattr(hip, "_lib", rec)
    hooks = []
    try:
        call = CASES[name](model)               # muted: a pipeline's constructor runs the chain too
        hooks = [model.register_forward_pre_hook(lambda m, a: setattr(rec, "muted", True)),
                 model.register_forward_hook(lambda m, a, out: setattr(rec, "muted", False))]
        rec.muted = False
        with torch.no_grad():
            call()
        rec.muted = True
        torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
        patch.undo()
    return rec.calls


@pytest.fixture(scope="module")
def model():
    return make_model()


@pytest.fixture(scope="module")
def expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu
def test_the_fixture_holds_every_case(expected):
    assert sorted(expected) == sorted(CASES) and all(len(v) > 0 for v in expected.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_c_calls_are_those_recorded_before_the_fold(name, model, expected, monkeypatch):
    got = json.loads(json.dumps(trace(name, model, monkeypatch)))
    print(name, "->", len(got), "calls:", sorted({c[0] for c in got}))
    assert len(got) > 0
    assert [c[0] for c in got] == [c[0] for c in expected[name]]
    assert got == expected[name]


if __name__ == "__main__":
    assert isinstance(hip._lib, ctypes.CDLL)
    the_model, out = make_model(), (sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
    traces = {}
    for case in CASES:
        with pytest.MonkeyPatch.context() as mp:
            traces[case] = trace(case, the_model, mp)
        print(case, "->", len(traces[case]), "calls")
        assert traces[case]
    with open(out, "w") as f:                   # one call per line
        f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(json.dumps(c) for c in v) + "\n]"
                                   for k, v in sorted(traces.items())) + "\n}\n")
    print("wrote", out)
