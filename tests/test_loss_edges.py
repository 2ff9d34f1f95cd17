"""The loss kernels (csrc/loss.hip) at their edges against the fp64 oracle (oracle/loss_oracle.py run on fp64 maps).

SimOTA is a chain of discrete decisions; the tests separate DECISIONS from VALUES.  Every detection case is built so
that each decision is decided at fp32 precision (LO.decision_margins; the CPU guard test_cases_reach_their_paths keeps
that true and also checks that each case reaches the path it is named after), so the kernel's assignment is compared
EXACTLY with the fp64 oracle's, and the values with a bound that comes from the reference's own arithmetic:

    bound = max(floor, 4 x distance(fp32 oracle, fp64 oracle))         distance = rel-to-max, as rel() in test_loss.py

The fp32 oracle is the reference's arithmetic.  The factor 4: the kernel sums the ~100 terms behind one anchor's loss
and gradient (up to 32 classes x a few operations, the IoU chain, fp32 exp/log of its own) in another order and with
another exp/log than torch's CPU kernels; rounding errors of n terms in a different order differ by a small multiple
of the error itself, never by an order of magnitude.  The floors are the project's existing bounds (loss 1e-5,
gradients 2e-5 in test_loss.py; 1e-6 for mean_square), so a case where fp32 torch happens to be exact does not ask the
kernel for better than fp32.  The kernel's own output never sets a bound."""
import functools

import numpy as np
import pytest
import torch

from oracle import loss_oracle as LO

FLOOR_LOSS, FLOOR_GRAD = 1e-5, 2e-5


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item() if b.numel() else 0.0


# =============================================================================================== detection cases
def _maps(rng, B, nc, shapes, wh_shift=0.0):
    """Head outputs like LO.synthetic_preds: N(0, 0.8), wh logits 0.4 N + 1 (boxes of a few strides)."""
    out = []
    for h, w in shapes:
        d = torch.from_numpy(rng.standard_normal((B, 5 + nc, h, w)).astype(np.float32) * 0.8)
        d[:, 2:4] = d[:, 2:4] * 0.5 + 1.0 + wh_shift
        out.append(d)
    return out


def _boxes(rng, n, W, H, nc, lo=40, hi=90, classes=None):
    """n boxes [cx, cy, w, h, cls] on a 1/4 px lattice (dyadic: the in-box / in-centre predicates are exact in fp32).
    Sides >= 40 px keep >= 25 anchors of the finest level inside 'box and centre', so the k <= 10 cheapest never reach
    into the costs that carry the +100000 penalty, where fp32 resolves only 1/128."""
    wh = rng.integers(lo * 4, hi * 4 + 1, (n, 2)) / 4.0
    c = np.stack([rng.integers(W, 3 * W + 1, n) / 4.0, rng.integers(H, 3 * H + 1, n) / 4.0], 1)
    cls = rng.integers(0, nc, (n, 1)) if classes is None else np.asarray(classes).reshape(n, 1)
    return torch.from_numpy(np.concatenate([c, wh, cls], 1).astype(np.float32)).reshape(n, 5)


def _constructed(B, h, w, s, nc, cell, box_wh, pred_c, seed):
    """One level, one box per image centred on the centre of `cell` = (gx, gy).  Each of the 25 candidates (the 5 x 5
    centre window) predicts a box of stride x stride (wh logits 0) centred at pred_c(b) -- x = cx / s - gx is dyadic, so
    prediction edges are exact in fp32 and fp64 alike.  All candidates of an image have the same IoU, so the order of
    their costs is set by the logit of the box's class, 0.6, 0.2, ... -9.0 in a shuffled order (cost steps >= 0.08): 24 of the 25 costs carry
    the penalty and differ by far more than the 1/64 fp32 resolves there."""
    rng = np.random.default_rng(seed)
    (m,) = _maps(rng, B, nc, [(h, w)])
    gx0, gy0 = cell
    labels = []
    for b in range(B):
        cx, cy = (gx0 + 0.5) * s, (gy0 + 0.5) * s
        labels.append(torch.tensor([[cx, cy, box_wh, box_wh, nc - 1]], dtype=torch.float32))
        px, py = pred_c(b, cx, cy)
        order = rng.permutation(25)
        for j, (dy, dx) in enumerate((dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)):
            gx, gy = gx0 + dx, gy0 + dy
            m[b, 0, gy, gx], m[b, 1, gy, gx] = px / s - gx, py / s - gy
            m[b, 2:4, gy, gx] = 0.0
            m[b, 4, gy, gx] = 1.0
            m[b, 5:, gy, gx] = -2.0
            m[b, 5 + nc - 1, gy, gx] = 0.6 - 0.4 * float(order[j])
    return [m], labels, [s], nc


def case_k10_exact():                   # every candidate's prediction IS the box: IoU 1 x 25, sum of the top ten = 10.0
    return _constructed(1, 8, 12, 16, 3, (5, 3), 16.0, lambda b, cx, cy: (cx, cy), seed=1)


def case_edge_tie():
    """Box 32 x 32 (edges c -+ 16), predictions 16 x 16: image b ties its left / top / right / bottom edge with the box's
    and differs in the other three; IoU 0.25 each, top-10 sum 2.5, k = 2."""
    off = [(-8.0, -2.0), (-2.0, -8.0), (8.0, 2.0), (2.0, 8.0)]
    return _constructed(4, 8, 8, 16, 2, (4, 4), 32.0, lambda b, cx, cy: (cx + off[b][0], cy + off[b][1]), seed=2)


def case_k_clamped_to_1():              # predictions of ~2 px against a 100 x 100 box: IoU sum far below 1
    rng = np.random.default_rng(3)
    return _maps(rng, 1, 4, [(8, 8)], wh_shift=-3.0), [torch.tensor([[64., 64., 100., 100., 1.]])], [16], 4


def case_few_candidates():
    """Box centred at (1, 1): its centre window holds the 2 x 2 corner anchors only.  The first selection loop breaks after
    4 of 10 rounds.  (The second loop's break needs k > candidates, and k <= sum of IoUs <= candidates: it can only fire
    with no candidate at all -- the case below.)"""
    rng = np.random.default_rng(4)
    return _maps(rng, 1, 4, [(4, 4)]), [torch.tensor([[1., 1., 40., 40., 2.]])], [32], 4


def case_no_candidates():               # image 0: one box far outside, no candidate at all; image 1 normal; image 2 empty
    rng = np.random.default_rng(5)
    labels = [torch.tensor([[-500., -500., 20., 20., 1.]]), _boxes(rng, 1, 128, 128, 4), torch.zeros(0, 5)]
    return _maps(rng, 3, 4, [(16, 16), (8, 8), (4, 4)]), labels, [8, 16, 32], 4


def case_nonsquare_levels():
    rng = np.random.default_rng(6)
    labels = [_boxes(rng, 3, 160, 96, 4, lo=40, hi=70), _boxes(rng, 2, 160, 96, 4, lo=40, hi=70)]
    return _maps(rng, 2, 4, [(12, 20), (6, 10), (3, 5)]), labels, [8, 16, 32], 4


def case_one_level():
    rng = np.random.default_rng(7)
    return _maps(rng, 2, 4, [(16, 16)]), [_boxes(rng, 2, 128, 128, 4), _boxes(rng, 3, 128, 128, 4)], [8], 4


_EIGHT = [(16, 16, 8), (8, 8, 16), (4, 4, 32), (2, 2, 64), (1, 1, 128), (8, 8, 16), (4, 4, 32), (2, 2, 64)]


def case_eight_levels():
    rng = np.random.default_rng(8)
    return (_maps(rng, 2, 4, [(h, w) for h, w, _ in _EIGHT]), [_boxes(rng, 2, 128, 128, 4), _boxes(rng, 1, 128, 128, 4)],
            [s for _, _, s in _EIGHT], 4)


def case_nc1():
    rng = np.random.default_rng(9)
    return _maps(rng, 2, 1, [(16, 16), (8, 8), (4, 4)]), [_boxes(rng, 2, 128, 128, 1), _boxes(rng, 2, 128, 128, 1)], [8, 16, 32], 1


def case_nc32():
    rng = np.random.default_rng(10)
    labels = [_boxes(rng, 2, 128, 128, 32, classes=[0, 31]), _boxes(rng, 2, 128, 128, 32, classes=[31, 17])]
    return _maps(rng, 2, 32, [(16, 16), (8, 8), (4, 4)]), labels, [8, 16, 32], 32


def case_anchor_limit():
    """128 x 256 cells of stride 8: 32768 anchors, all 1024 words of the `taken` bit mask.  The third box sits in the
    bottom-right corner: its matches are in the last word (anchor index >= 32736)."""
    rng = np.random.default_rng(11)
    labels = torch.tensor([[300., 200., 64., 48., 0.], [1000.5, 512.25, 80., 120., 1.], [2020., 1004., 48., 40., 1.]])
    return _maps(rng, 1, 2, [(128, 256)]), [labels], [8], 2


def case_crowded():
    """300 / 0 / 1 boxes on 128 px, centres within the middle half: every anchor near the middle is claimed by many boxes.
    Boxes 2 and 200 of image 0 are bit-identical: they select the same anchors, and each of those goes to box 2 unless a
    third box is cheaper."""
    rng = np.random.default_rng(12)
    many = _boxes(rng, 300, 128, 128, 4)
    many[200] = many[2]
    return _maps(rng, 3, 4, [(16, 16), (8, 8), (4, 4)]), [many, torch.zeros(0, 5), _boxes(rng, 1, 128, 128, 4)], [8, 16, 32], 4


def case_saturated():
    """obj and cls logits from {-50, -12, 12, 50}.  +-12 is unsaturated in fp32 and stresses the logs (1 - sigmoid(12) =
    6e-6); +-50 saturates fp32 and fp64 alike (sigmoid == 1 or 2e-22), so both take the -100 clamp of BCE's logs where
    cls = obj = 50.  Values in between are avoided: there fp32 and fp64 legitimately differ."""
    rng = np.random.default_rng(13)
    maps = _maps(rng, 2, 4, [(16, 16), (8, 8), (4, 4)])
    vals = torch.tensor([-50., -12., 12., 50.])
    for m in maps:
        m[:, 4:] = vals[torch.from_numpy(rng.integers(0, 4, tuple(m[:, 4:].shape)))]
    return maps, [_boxes(rng, 2, 128, 128, 4), _boxes(rng, 2, 128, 128, 4)], [8, 16, 32], 4


# name -> builder.  Measured distance of the fp32 oracle from the fp64 oracle (rel-to-max; loss / worst of the three
# component sums / worst level's gradient / matched IoUs), from which the kernel's bounds follow as described on top:
DET_CASES = {
    "k10_exact": case_k10_exact,                # 2.8e-09 / 2.8e-08 / 6.4e-08 / 0.0e+00
    "k_clamped_to_1": case_k_clamped_to_1,      # 1.6e-08 / 3.1e-08 / 6.3e-08 / 5.9e-07
    "few_candidates": case_few_candidates,      # 5.6e-08 / 5.6e-08 / 5.3e-08 / 1.6e-07
    "no_candidates": case_no_candidates,        # 3.0e-08 / 5.3e-08 / 1.3e-07 / 7.0e-08
    "edge_tie": case_edge_tie,                  # 4.5e-08 / 1.0e-07 / 7.4e-08 / 0.0e+00
    "nonsquare_levels": case_nonsquare_levels,  # 4.4e-08 / 1.4e-07 / 2.7e-07 / 1.7e-07
    "one_level": case_one_level,                # 2.3e-08 / 6.6e-08 / 2.1e-07 / 4.6e-07
    "eight_levels": case_eight_levels,          # 1.8e-08 / 4.0e-08 / 3.6e-07 / 3.2e-07
    "nc1": case_nc1,                            # 6.3e-10 / 8.7e-08 / 1.2e-07 / 1.4e-07
    "nc32": case_nc32,                          # 9.9e-09 / 6.4e-08 / 2.4e-07 / 3.6e-07
    "anchor_limit": case_anchor_limit,          # 3.9e-08 / 2.2e-07 / 1.2e-06 / 1.1e-06
    "crowded": case_crowded,                    # 3.8e-08 / 6.6e-08 / 3.1e-07 / 3.0e-07
    "saturated": case_saturated,                # 1.1e-07 / 1.1e-07 / 1.1e-07 / 3.0e-07
}


def _oracle_run(maps, labels, strides, nc, dtype):
    ins = [m.clone().to(dtype).requires_grad_(True) for m in maps]          # never the cached tensor itself
    loss, assigns, comps = LO.yolo_loss(ins, labels, nc, strides=strides, return_assignment=True, return_components=True)
    loss.backward()
    return dict(loss=loss.detach(), assigns=assigns, grads=[i.grad for i in ins], nfg=comps[3],
                comps=torch.stack([c.detach() for c in comps[:3]]),
                piou=torch.cat([a[2] for a in assigns]))


@functools.lru_cache(maxsize=None)
def det_case(name):
    """The case's inputs, its fp64 oracle, and the distance of the fp32 oracle from it: computed once, shared, read-only."""
    maps, labels, strides, nc = DET_CASES[name]()
    o64, o32 = _oracle_run(maps, labels, strides, nc, torch.float64), _oracle_run(maps, labels, strides, nc, torch.float32)
    same = all(torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) for a, c in zip(o64["assigns"], o32["assigns"]))
    d32 = dict(same_assignment=same, loss=rel(o32["loss"], o64["loss"]),
               comps=max(rel(o32["comps"][i], o64["comps"][i]) for i in range(3)),
               grad=max(rel(a, c) for a, c in zip(o32["grads"], o64["grads"])),
               piou=rel(o32["piou"], o64["piou"]) if same else float("nan"))
    return dict(maps=maps, labels=labels, strides=strides, nc=nc, o64=o64, d32=d32)


def bounds(d32):
    return dict(loss=max(FLOOR_LOSS, 4 * d32["loss"]), comps=max(FLOOR_LOSS, 4 * d32["comps"]),
                grad=max(FLOOR_GRAD, 4 * d32["grad"]), piou=max(FLOOR_LOSS, 4 * d32["piou"]))


# ------------------------------------------------------------------------------------------------ CPU guard
def _matched_anchors(assigns, b):
    return assigns[b][0].nonzero().flatten()


def _reaches(name, c, mg):
    """What the case is in the table for, asserted from the oracle alone."""
    o, maps, labels = c["o64"], c["maps"], c["labels"]
    if name == "k10_exact":
        assert mg[0]["k"] == [10] and o["nfg"] == 10 and mg[0]["n_candidates"] == 25 and mg[0]["iou_sum"] == [10.0]
    elif name == "k_clamped_to_1":
        assert mg[0]["k"] == [1] and mg[0]["iou_sum"][0] < 1.0 and int(mg[0]["iou_sum"][0]) == 0 and o["nfg"] == 1
    elif name == "few_candidates":
        assert 0 < mg[0]["n_candidates"] < 10 and o["nfg"] >= 1
    elif name == "no_candidates":
        assert mg[0]["n_candidates"] == 0 and mg[0]["k"] == [0] and not o["assigns"][0][0].any()
        assert mg[1]["n_candidates"] > 0 and o["assigns"][1][0].any() and mg[2] is None
    elif name == "edge_tie":
        out, _, _, _ = LO.decode_levels([m.double() for m in maps], c["strides"])
        moved = 0
        for b in range(len(labels)):
            fgi = _matched_anchors(o["assigns"], b)
            assert len(fgi) == 2
            p, g = out[b, fgi, :4], labels[b][0, :4].double()
            pe = torch.stack([p[:, 0] - p[:, 2] / 2, p[:, 1] - p[:, 3] / 2, p[:, 0] + p[:, 2] / 2, p[:, 1] + p[:, 3] / 2], 1)
            ge = torch.stack([g[0] - g[2] / 2, g[1] - g[3] / 2, g[0] + g[2] / 2, g[1] + g[3] / 2])
            assert ((pe == ge).sum(1) == 1).all() and ((pe == ge).sum(0) > 0).tolist() == [b == 0, b == 1, b == 2, b == 3]
            gy, gx = fgi // maps[0].shape[3], fgi % maps[0].shape[3]
            # the gradient along the tied axis is HALF of what the untied side alone would give -- not 0 (both sides to the
            # prediction) and not the whole: non-zero position gradient on that axis, and non-zero size gradients
            moved += int((o["grads"][0][b][[b % 2, 2, 3]][:, gy, gx] != 0).all(0).sum())
        assert moved == 2 * len(labels)
    elif name == "nonsquare_levels":
        assert all(m.shape[2] != m.shape[3] for m in maps) and o["nfg"] > 0
        a0 = 0
        for m in maps:                                      # every level takes part, beyond its first row
            hw = m.shape[2] * m.shape[3]
            assert any(((f := _matched_anchors(o["assigns"], b)) >= a0 + m.shape[3]).logical_and(f < a0 + hw).any() for b in range(2))
            a0 += hw
    elif name == "one_level":
        assert len(maps) == 1 and o["nfg"] > 0
    elif name == "eight_levels":
        assert len(maps) == 8 and o["nfg"] > 0
        a0 = np.cumsum([0] + [m.shape[2] * m.shape[3] for m in maps])
        f = torch.cat([_matched_anchors(o["assigns"], b) for b in range(2)])
        hit = [bool(((f >= a0[l]) & (f < a0[l + 1])).any()) for l in range(8)]
        # matches before and after the 1 x 1 level in the middle (unmatched levels still carry objectness loss and gradient)
        assert sum(hit) >= 5 and any(hit[:4]) and any(hit[5:]), hit
    elif name == "nc1":
        assert c["nc"] == 1 and o["nfg"] > 0
    elif name == "nc32":
        cls = torch.cat([l[:, 4] for l in labels])
        assert c["nc"] == 32 and (cls == 0).any() and (cls == 31).any() and o["nfg"] > 0
        assert 31 in labels[0][o["assigns"][0][1], 4].tolist()           # class NC-1 is matched, not only present
    elif name == "anchor_limit":
        fgi = _matched_anchors(o["assigns"], 0)
        assert sum(m.shape[2] * m.shape[3] for m in maps) == 32768 and (fgi >= 32736).any() and (fgi < 32).sum() == 0
        assert set(o["assigns"][0][1].tolist()) == {0, 1, 2}
    elif name == "crowded":
        assert [len(l) for l in labels] == [300, 0, 1] and mg[0]["ambiguous"] >= 50
        assert torch.equal(labels[0][2], labels[0][200])
        m = o["assigns"][0][1]
        assert (m == 2).any() and not (m == 200).any()       # the duplicates' shared anchors go to the lower index
    elif name == "saturated":
        assert all(set(m[:, 4:].unique().tolist()) == {-50., -12., 12., 50.} for m in maps) and o["nfg"] > 0
        clamp = False
        for b in range(2):                                   # a candidate with cls = obj = 50: the cost's log clamp
            out = torch.cat([m[b].flatten(1).t() for m in maps])
            cand = LO.in_boxes_info(labels[b][:, :4], *_grid(maps, c["strides"]))[0]
            clamp |= bool(((out[cand, 4:5] == 50) & (out[cand, 5:] == 50)).any())
        assert clamp
        fgc = torch.cat([torch.cat([m[b].flatten(1).t() for m in maps])[o["assigns"][b][0]] for b in range(2)])
        assert (fgc[:, 4:].abs() == 50).any()                # saturated logits in the loss terms of foreground anchors
    else:
        raise AssertionError(name)


def _grid(maps, strides):
    _, xs, ys, ss = LO.decode_levels(maps, strides)
    return ss, xs, ys


@pytest.mark.parametrize("name", list(DET_CASES))
def test_cases_reach_their_paths(name):
    """CPU guard of the case table: the case reaches what it is named after, and EVERY decision of its assignment is
    decided at fp32 precision (LO.decision_margins) -- the condition under which an exact comparison of the kernel's
    assignment with the fp64 oracle's is legitimate.  The fp32 oracle must then take the same decisions."""
    c = det_case(name)
    mg = LO.decision_margins(c["maps"], c["labels"], c["nc"], c["strides"])
    print(name, "fp32 oracle vs fp64 oracle:", c["d32"])
    for b, r in enumerate(mg):
        if r is not None:
            print(name, "image", b, {k: (v if not isinstance(v, list) or len(v) < 12 else f"{len(v)} values, min "
                                         f"{min((x for x in v if x is not None), default=None)}") for k, v in r.items()})
            assert r["undecided"] == [], (name, b, r["undecided"])
    _reaches(name, c, mg)
    assert c["d32"]["same_assignment"]
    assert all(torch.isfinite(g).all() for g in c["o64"]["grads"]) and torch.isfinite(c["o64"]["loss"])


# ------------------------------------------------------------------------------------------------ GPU: detection
def _kernel(c, grads=True):
    from asy_vrnet_amd import losses
    yl = losses.YOLOLoss(c["nc"], strides=c["strides"]).cuda()
    ins = [m.clone().cuda().requires_grad_(grads) for m in c["maps"]]
    loss = yl(ins, c["labels"])
    stats = yl.last_stats
    if grads:
        loss.backward()
    return yl, loss.detach(), stats, [i.grad for i in ins]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DET_CASES))
def test_assignment_matches_fp64_oracle(name):
    c = det_case(name)
    from asy_vrnet_amd import losses
    yl = losses.YOLOLoss(c["nc"], strides=c["strides"]).cuda()
    fg, mg, pi, stats = yl.assignments([m.cuda() for m in c["maps"]], c["labels"])
    fg, mg, pi = fg.cpu(), mg.cpu(), pi.cpu()
    bound = bounds(c["d32"])["piou"]
    for b, (ofg, omatched, opious) in enumerate(c["o64"]["assigns"]):
        assert torch.equal(fg[b], ofg), (name, b, (fg[b] != ofg).nonzero().flatten().tolist())
        assert torch.equal(mg[b][ofg].long(), omatched), (name, b)
        d = rel(pi[b][ofg], opious)
        print(name, "image", b, "pred_iou distance", d, "bound", bound)
        assert d <= bound, (name, b, d, bound)
        assert (mg[b][~ofg] == -1).all() and (pi[b][~ofg] == 0).all()
    assert int(stats[1].item()) == c["o64"]["nfg"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DET_CASES))
def test_values_match_fp64_oracle(name):
    """Loss, the three component sums of last_stats and every level's gradient; the value-only call returns the same five
    numbers bit for bit; a second call repeats loss, stats and gradients bit for bit."""
    c = det_case(name)
    o, bd = c["o64"], bounds(c["d32"])
    yl, loss, stats, grads = _kernel(c)
    stats = stats.cpu()
    d_loss, d_comp = rel(loss.cpu(), o["loss"]), [rel(stats[2 + i], o["comps"][i]) for i in range(3)]
    d_grad = [rel(g.cpu(), og) for g, og in zip(grads, o["grads"])]
    print(name, "fp32 oracle:", c["d32"], "bounds:", bd)
    print(name, "KERNEL loss", d_loss, "components", d_comp, "gradients", d_grad)
    assert torch.equal(stats[0], loss.cpu()) and int(stats[1]) == o["nfg"]
    assert d_loss <= bd["loss"], (name, d_loss, bd["loss"])
    assert max(d_comp) <= bd["comps"], (name, d_comp, bd["comps"])
    assert max(d_grad) <= bd["grad"], (name, d_grad, bd["grad"])
    assert all(torch.isfinite(g).all() for g in grads)
    if name == "edge_tie":                                  # the matched anchors' box gradients are not identically zero
        for b in range(len(c["labels"])):
            fgi = _matched_anchors(o["assigns"], b)
            gy, gx = fgi // c["maps"][0].shape[3], fgi % c["maps"][0].shape[3]
            assert (grads[0][b][[b % 2, 2, 3]][:, gy, gx] != 0).all()
    # value-only path
    _, loss0, _, _ = _kernel(c, grads=False)
    _, _, _, stats0 = yl.assignments([m.cuda() for m in c["maps"]], c["labels"])
    assert torch.equal(loss0, loss) and torch.equal(stats0.cpu(), stats)
    # repeatability
    _, loss2, stats2, grads2 = _kernel(c)
    assert torch.equal(loss2, loss) and torch.equal(stats2.cpu(), stats)
    assert all(torch.equal(a, b_) for a, b_ in zip(grads2, grads))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DET_CASES))
def test_padding_slots_are_never_read(name):
    """forward_packed with max_gt above every count: NaN in the unused slots gives bit for bit what zeros give."""
    from asy_vrnet_amd import losses
    c = det_case(name)
    B, counts = len(c["labels"]), [len(l) for l in c["labels"]]
    G = max(counts) + 3
    res = []
    for fill in (0.0, float("nan")):
        packed = torch.full((B, G, 5), fill, dtype=torch.float32)
        for b, l in enumerate(c["labels"]):
            packed[b, :counts[b]] = l
        yl = losses.YOLOLoss(c["nc"], strides=c["strides"]).cuda()
        ins = [m.clone().cuda().requires_grad_(True) for m in c["maps"]]
        loss = yl.forward_packed(ins, packed.cuda(), torch.tensor(counts, dtype=torch.int32).cuda(), G)
        loss.backward()
        res.append((loss.detach(), yl.last_stats.clone(), [i.grad for i in ins]))
    (l0, s0, g0), (l1, s1, g1) = res
    assert torch.isfinite(l1) and torch.equal(l0, l1) and torch.equal(s0, s1)
    assert all(torch.equal(a, b_) for a, b_ in zip(g0, g1))
    assert rel(l0.cpu(), c["o64"]["loss"]) <= bounds(c["d32"])["loss"]


@pytest.mark.gpu
def test_detection_limits_are_rejected():
    from asy_vrnet_amd import losses
    box = [torch.tensor([[32., 32., 40., 40., 0.]])]
    nine = [torch.zeros(1, 9, 8, 8).cuda() for _ in range(9)]
    with pytest.raises(RuntimeError):
        losses.YOLOLoss(4, strides=[8] * 9).cuda()(nine, box)
    losses.YOLOLoss(4, strides=[8] * 8).cuda()(nine[:8], box)                  # 8 levels are accepted
    with pytest.raises(RuntimeError):
        losses.YOLOLoss(33, strides=[8]).cuda()([torch.zeros(1, 38, 8, 8).cuda()], box)
    big = [torch.zeros(1, 7, 128, 256).cuda(), torch.zeros(1, 7, 1, 1).cuda()]
    with pytest.raises(RuntimeError):
        losses.YOLOLoss(2, strides=[8, 2048]).cuda()(big, box)                 # 32769 anchors
    torch.cuda.synchronize()


# =============================================================================================== segmentation
def _seg_inputs(B, C, H, W, seed, ignore=0.15, absent=None, all_ignored=False, confident=False, weights=True):
    rng = np.random.default_rng([seed, B, C, H, W])
    x = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32) * 1.5)
    png = rng.integers(0, C, (B, H, W))
    if absent is not None:
        png[png == absent] = (absent + 1) % C
    png[rng.random((B, H, W)) < ignore] = C
    if all_ignored:
        png[:] = C
    if confident:                                           # x_t = 50, the others 0: p_t == 1 in fp32, 1 - pt == 0
        x = torch.zeros(B, C, H, W)
        t = torch.from_numpy(np.where(png == C, 0, png))
        x.scatter_(1, t[:, None], 50.0)
    onehot = torch.from_numpy(np.eye(C + 1, dtype=np.float32)[png])
    w = torch.from_numpy(rng.uniform(0.5, 2.0, C).astype(np.float32)) if weights else None
    return x, torch.from_numpy(png.astype(np.int64)), onehot, w


# name -> (inputs, loss parameters).  Measured distance of the fp32 oracle from the fp64 oracle, loss / gradient per mode (all
# below a quarter of the floors, so the floors 1e-5 / 2e-5 are the kernel's bounds throughout):
#   px1          ce 4.9e-08 / 8.5e-09  focal 3.7e-08 / 3.0e-08  dice 4.3e-10 / 1.6e-07  train 1.4e-08 / 3.4e-08
#   px65         ce 2.5e-07 / 1.4e-07  focal 5.8e-08 / 1.2e-07  dice 6.8e-08 / 1.6e-07  train 1.1e-07 / 1.4e-07
#   px1023       ce 1.2e-07 / 2.2e-07  focal 1.3e-07 / 2.0e-07  dice 5.4e-08 / 3.4e-07  train 6.2e-08 / 2.2e-07
#   c1           ce 0 / 0              focal 0 / 0              dice 1.1e-06 / 0        train 1.1e-06 / 0
#   c32          ce 1.5e-07 / 9.0e-08  focal 5.1e-08 / 1.6e-07  dice 1.4e-09 / 2.0e-07  train 2.1e-08 / 1.5e-07
#   all_ignored  ce NaN == NaN / 0     focal 0 / 0              dice 2.9e-08 / 4.2e-07  train 1.8e-08 / 3.8e-07
#   class_absent ce 8.2e-08 / 2.1e-07  focal 4.1e-08 / 2.7e-07  dice 3.6e-08 / 2.3e-07  train 3.9e-08 / 1.8e-07
#   confident    ce 0 / 5.6e-19        focal 0 / 0              dice 2.8e-07 / 8.3e-19  train 2.8e-07 / 2.3e-18
#   params       ce 9.0e-08 / 1.3e-07  focal 1.6e-08 / 2.2e-07  dice 1.7e-08 / 1.6e-07  train 1.5e-08 / 1.6e-07
#   no_weights   ce 1.6e-08 / 1.3e-07  focal 7.8e-08 / 1.8e-07  dice 4.4e-08 / 3.0e-07  train 9.3e-08 / 1.4e-07
#   capped       ce 9.9e-08 / 1.4e-07  focal 6.5e-09 / 3.0e-07  dice 1.6e-08 / 4.7e-07  train 1.1e-08 / 3.1e-07
SEG_CASES = {
    "px1": (lambda: _seg_inputs(1, 3, 1, 1, 1, ignore=0.0), {}),
    "px65": (lambda: _seg_inputs(1, 3, 1, 65, 2), {}),
    "px1023": (lambda: _seg_inputs(1, 3, 3, 341, 3), {}),
    "c1": (lambda: _seg_inputs(2, 1, 5, 7, 4), {}),
    "c32": (lambda: _seg_inputs(1, 32, 9, 13, 5), {}),                # SMAXC: 99 fp64 accumulators per thread
    "all_ignored": (lambda: _seg_inputs(1, 3, 4, 5, 6, all_ignored=True), {}),
    "class_absent": (lambda: _seg_inputs(2, 4, 6, 9, 7, ignore=0.0, absent=2), {}),
    "confident": (lambda: _seg_inputs(1, 3, 6, 7, 8, confident=True), {}),
    "params": (lambda: _seg_inputs(2, 5, 7, 9, 9), dict(alpha=None, gamma=3, beta=2, smooth=1)),
    "no_weights": (lambda: _seg_inputs(2, 4, 6, 9, 10, weights=False), {}),
    "capped": (lambda: _seg_inputs(1, 2, 1449, 1449, 11), {}),        # 2 099 601 pixels > 2048 x 1024: 2048 workgroups
}
SEG_MODES = ("ce", "focal", "dice", "train")


def _seg_oracle(mode, x, png, onehot, w, prm, dtype):
    C = x.shape[1]
    x = x.clone().to(dtype).requires_grad_(True)
    w = None if w is None else w.to(dtype)
    fo = lambda: LO.focal_loss(x, png, w, C, alpha=prm.get("alpha", 0.5), gamma=prm.get("gamma", 2))
    di = lambda: LO.dice_loss(x, onehot.to(dtype), beta=prm.get("beta", 1), smooth=prm.get("smooth", 1e-5))
    loss = {"ce": lambda: LO.ce_loss(x, png, w, C), "focal": fo, "dice": di, "train": lambda: 5 * (fo() + di())}[mode]()
    loss.backward()
    return loss.detach(), x.grad


def _seg_kernel(mode, x, png, onehot, w, prm):
    from asy_vrnet_amd import losses
    C = x.shape[1]
    x = x.clone().cuda().requires_grad_(True)
    png, onehot, w = png.cuda(), onehot.cuda(), None if w is None else w.cuda()
    fa = dict(alpha=prm.get("alpha", 0.5), gamma=prm.get("gamma", 2))
    da = dict(beta=prm.get("beta", 1), smooth=prm.get("smooth", 1e-5))
    if mode == "ce":
        loss = losses.CE_Loss(x, png, w, num_classes=C)
    elif mode == "focal":
        loss = losses.Focal_Loss(x, png, w, num_classes=C, **fa)
    elif mode == "dice":
        loss = losses.Dice_loss(x, onehot, **da)
    else:                                                   # training_loss's seg term: Focal + Dice, factor 5 in the kernel
        loss = losses._seg(x, png, onehot, w, focal=True, dice=True, alpha=1.0 if fa["alpha"] is None else fa["alpha"],
                           gamma=fa["gamma"], scale=5.0, **da)
    loss.backward()
    return loss.detach(), x.grad


@functools.lru_cache(maxsize=None)
def seg_case(name, mode):
    build, prm = SEG_CASES[name]
    inp = build()
    l64, g64 = _seg_oracle(mode, *inp, prm, torch.float64)
    l32, g32 = _seg_oracle(mode, *inp, prm, torch.float32)
    nan = bool(torch.isnan(l64))
    d32 = dict(loss=0.0 if nan else rel(l32, l64), grad=0.0 if nan else rel(g32, g64))
    return inp, prm, l64, g64, d32


@pytest.mark.parametrize("name", list(SEG_CASES))
def test_seg_cases_reach_their_paths(name):
    """CPU guard of the seg table, from the inputs and the oracle alone."""
    x, png, onehot, w = SEG_CASES[name][0]()
    B, C, H, W = x.shape
    n = B * H * W
    want = dict(px1=1, px65=65, px1023=1023, capped=1449 * 1449)
    if name in want:
        assert n == want[name]
    assert n % 64 != 0 or name not in ("px1", "px65", "px1023", "capped")
    if name == "capped":
        assert n > 2048 * 1024 and -(-n // (2048 * 256)) > 4           # more than the usual four grid-stride trips
    if name in ("c1", "c32"):
        assert C == int(name[1:])
    if name == "all_ignored":
        assert (png == C).all()
        assert torch.isnan(seg_case(name, "ce")[2]) and seg_case(name, "focal")[2] == 0
    elif name != "px1":
        assert (png != C).any()
    if name == "class_absent":
        assert not (png == 2).any() and not (png == C).any() and all((png == c).any() for c in (0, 1, 3))
    if name == "confident":
        p = torch.softmax(x, 1).gather(1, png.clamp_max(C - 1)[:, None])
        assert (p[(png != C)[:, None]] == 1).all() and (x.max() == 50)                      # 1 - pt == 0 in fp32
        assert all(torch.isfinite(seg_case(name, m)[3]).all() for m in SEG_MODES)
    if name == "params":
        assert SEG_CASES[name][1] == dict(alpha=None, gamma=3, beta=2, smooth=1)
    if name == "no_weights":
        assert w is None
    for m in SEG_MODES:
        print(name, m, "fp32 oracle vs fp64 oracle:", seg_case(name, m)[4])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", SEG_MODES)
@pytest.mark.parametrize("name", list(SEG_CASES))
def test_seg_matches_fp64_oracle(name, mode):
    inp, prm, l64, g64, d32 = seg_case(name, mode)
    b_loss, b_grad = max(FLOOR_LOSS, 4 * d32["loss"]), max(FLOOR_GRAD, 4 * d32["grad"])
    loss, grad = _seg_kernel(mode, *inp, prm)
    loss, grad = loss.cpu(), grad.cpu()
    if torch.isnan(l64):                                    # CE over no pixel at all: 0 / 0 in oracle and kernel alike
        assert torch.isnan(loss)
        if (g64 == 0).all():
            assert (grad == 0).all()
    else:
        d_loss, d_grad = rel(loss, l64), rel(grad, g64)
        print(name, mode, "fp32 oracle", d32, "bounds", (b_loss, b_grad), "KERNEL loss", d_loss, "gradient", d_grad)
        assert torch.isfinite(loss) and torch.isfinite(grad).all()
        assert d_loss <= b_loss, (name, mode, d_loss, b_loss)
        assert d_grad <= b_grad, (name, mode, d_grad, b_grad)
    loss2, grad2 = _seg_kernel(mode, *inp, prm)             # repeatable bit for bit
    assert torch.equal(loss2.cpu(), loss) or (torch.isnan(loss) and torch.isnan(loss2))
    assert torch.equal(grad2.cpu(), grad)


@pytest.mark.gpu
def test_seg_limits_are_rejected():
    from asy_vrnet_amd import losses
    x, png, onehot, _ = _seg_inputs(1, 33, 2, 3, 12)
    with pytest.raises(RuntimeError):
        losses.CE_Loss(x.cuda(), png.cuda(), None, num_classes=33)
    with pytest.raises(RuntimeError):
        losses.Dice_loss(x.cuda(), onehot.cuda())
    x, png, onehot, _ = _seg_inputs(2, 4, 3, 5, 13)
    with pytest.raises(RuntimeError):
        losses.Dice_loss(x.cuda(), onehot[..., :4].contiguous().cuda())          # (B, H, W, C): wrong last dimension
    torch.cuda.synchronize()


# =============================================================================================== mean_square
@pytest.mark.gpu
def test_mean_square_sizes_and_tensor_count():
    """Tensor sizes 1, 4095, 4097 around the 4096 elements of one workgroup, k = 8 tensors (MS_MAX); k = 9 is rejected."""
    from asy_vrnet_amd.losses import mean_square_loss
    g = torch.Generator().manual_seed(5)
    sizes = [1, 4095, 4097, 4096, 3, 8193, 255, 257]
    host = [torch.randn(n, generator=g) for n in sizes]

    def expr(dtype):
        ts = [t.clone().to(dtype).requires_grad_() for t in host]
        v = sum((t * t).mean() for t in ts)
        (v * 0.7).backward()
        return v.detach(), [t.grad for t in ts]
    v64, g64 = expr(torch.float64)
    v32, g32 = expr(torch.float32)
    b_val = max(1e-6, 4 * rel(v32, v64))
    b_grad = max(1e-6, 4 * max(rel(a, b) for a, b in zip(g32, g64)))
    ts = [t.cuda().requires_grad_() for t in host]
    got = mean_square_loss(ts[:7], ts[7])
    (got * 0.7).backward()
    d_val, d_grad = rel(got.detach().cpu(), v64), [rel(t.grad.cpu(), b) for t, b in zip(ts, g64)]
    print("mean_square bounds", (b_val, b_grad), "KERNEL value", d_val, "gradients", d_grad)
    assert d_val <= b_val and max(d_grad) <= b_grad
    assert torch.equal(mean_square_loss([t.detach() for t in ts[:7]], ts[7].detach()), got.detach())
    with pytest.raises(RuntimeError):
        mean_square_loss([t.detach() for t in ts] , ts[0].detach())             # 9 tensors
    torch.cuda.synchronize()
