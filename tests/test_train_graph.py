"""graph.TrainStep on the GPU: the captured training step (forward, the reference's loss, backward, optimizer step, EMA)
against the eager loop, bit for bit -- the `_dev` update kernels share their arithmetic with the scalar forms, the packed
loss runs the same kernels on a fixed-shape target buffer, and the graphs replay the eager step's launches.  Every
comparison is torch.equal.  Shapes: nano, 64 x 64, B = 2 (84 anchors; BatchNorm needs B >= 2)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S, NC, NS = 2, 64, 4, 9
SIZES = (1, 255, 256, 4096, 4097, 2 * 4096 + 3)          # a chunk edge (4096), a tail, a sub-wave tail


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import asy_vrnet_amd
    return asy_vrnet_amd


def rnd(n, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)).cuda()


def record(lr=0.0, decay=0.0, bc=(1.0, 1.0)):
    return torch.tensor([lr, decay, bc[0], bc[1]], dtype=torch.float32).cuda()


def tensors_equal(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


# ---- 1. the _dev forms against the scalar forms ------------------------------------------------------------------------
def make_optimizer(kind, seed):
    from asy_vrnet_amd import optim
    ps = [torch.nn.Parameter(rnd(n, seed + i)) for i, n in enumerate(SIZES)]
    if kind == "sgd":
        opt = optim.SGD(ps[0::2], 1e-2, momentum=0.937, nesterov=True)
    else:
        opt = optim.Adam(ps[0::2], 1e-3, betas=(0.937, 0.999))
    opt.add_param_group({"params": ps[1::2], "weight_decay": 5e-4})          # mixed zero and non-zero weight decay
    return ps, opt


def set_grads(ps, seed):
    for i, p in enumerate(ps):
        p.grad = rnd(p.numel(), seed + i, 0.1)


def optimizer_state_equal(ps, opt, qs, opt2):
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
        assert tensors_equal(opt.state[p], opt2.state[q])


def test_sgd_dev_equals_the_scalar_form(A):
    (ps, opt), (qs, opt2) = make_optimizer("sgd", 10), make_optimizer("sgd", 10)
    for it, lr in enumerate((1e-2, 3.7e-3, 3.7e-3)):                          # momentum buffers at zero, then in use
        for g in opt.param_groups + opt2.param_groups:
            g["lr"] = lr
        set_grads(ps, 100 + 10 * it)
        set_grads(qs, 100 + 10 * it)
        opt.step()
        opt2.step(scalars=record(lr=lr))
        optimizer_state_equal(ps, opt, qs, opt2)
    assert not torch.equal(ps[3], rnd(SIZES[3], 13))                          # the steps did move the parameters


def test_adam_dev_equals_the_scalar_form_at_step_1_and_7(A):
    (ps, opt), (qs, opt2) = make_optimizer("adam", 20), make_optimizer("adam", 20)
    for it, first in enumerate((0, 6)):
        for o, params in ((opt, ps), (opt2, qs)):
            set_grads(params, 200 + 10 * it)
            if first:
                for p in params:
                    o.state[p]["step"] = first
        opt.step()
        bc = opt2.advance()
        assert bc == A.hip.adam_bias_correction(0.937, 0.999, first + 1)
        opt2.step(scalars=record(lr=1e-3, bc=bc))
        assert all(opt2.state[q]["step"] == first + 1 for q in qs)
        optimizer_state_equal(ps, opt, qs, opt2)


@pytest.mark.parametrize("decay", [0.0, 0.63])
def test_ema_dev_equals_the_scalar_form(A, decay):
    from asy_vrnet_amd import optim

    class Bag(torch.nn.Module):
        def __init__(self, seed):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(rnd(n, seed + i)) for i, n in enumerate(SIZES)])
    live = Bag(30)
    e1, e2 = (optim.ModelEMA(Bag(40), decay=decay, tau=1e-9) for _ in range(2))       # tau -> 0: the ramp is `decay` at once
    for it in range(2):
        with torch.no_grad():
            for p in live.ps:
                p.add_(0.25)
        e1.update(live)
        d = e2.advance()
        assert d == np.float32(decay)
        e2.update(live, scalars=record(decay=d))
        assert e1.updates == e2.updates == it + 1
        assert tensors_equal(e1.ema.state_dict(), e2.ema.state_dict())
    if decay == 0.0:
        assert all(torch.equal(a, b) for a, b in zip(e2.ema.ps, live.ps))


# ---- 2. the packed loss against the list form ---------------------------------------------------------------------------
def test_forward_packed_equals_forward(A):
    from asy_vrnet_amd import losses
    from oracle import loss_oracle as LO
    seed = next(s for s in range(100) if LO.synthetic_targets(B, S, NC, NS, s, empty=(1,))[0][0].shape[0] == 3)
    labels = LO.synthetic_targets(B, S, NC, NS, seed, empty=(1,))[0]
    assert [int(l.shape[0]) for l in labels] == [3, 0]
    dets = [d.cuda() for d in LO.synthetic_preds(B, S, NC, NS, 3)[0]]
    out = []
    for packed in (False, True):
        yl = losses.YOLOLoss(NC).cuda()
        maps = [d.clone().requires_grad_(True) for d in dets]
        if packed:
            host, cnt = losses.pack_targets(labels, 8)
            loss = yl.forward_packed(maps, host.cuda(), cnt.cuda(), 8)
        else:
            loss = yl(maps, labels)                                               # G = the largest count, 3
        loss.backward()
        out.append((loss.detach(), yl.last_stats.clone(), [m.grad for m in maps]))
    (l0, s0, g0), (l1, s1, g1) = out
    assert torch.isfinite(l0) and s0[1] > 0                                       # there are foreground anchors
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


# ---- 3. the captured step against the eager loop ------------------------------------------------------------------------
def build(A, dtype="f32", seed=5):
    m = A.EfficientVRNet(NC, NS, "nano", img_size=(S, S)).cuda().train()
    A.randomize_state_dict(m.state_dict(), seed=seed)
    m.compute_dtype = dtype
    return m


def trainer(A, kind, dtype="f32", net_of=None):
    from asy_vrnet_amd import losses, optim
    m = build(A, dtype)
    opt = optim.build_optimizer(m, kind, 1e-2 if kind == "sgd" else 1e-3, 0.937, 5e-4)
    ema = optim.ModelEMA(m)
    return (m if net_of is None else net_of(m)), m, losses.YOLOLoss(NC).cuda(), opt, ema


def batch_of(A, seed):
    from oracle import loss_oracle as LO
    x, r = A.synthetic_inputs(B, S, seed, "cuda")
    labels, pngs, seg_labels = LO.synthetic_targets(B, S, NC, NS, seed, empty=(1,))
    return x, r, labels, pngs, seg_labels


def trainers_equal(a, b, what, optimizer_state=True):
    (_, m1, _, o1, e1), (_, m2, _, o2, e2) = a, b
    for (k, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), (what, k)
    for (k, p), (_, q) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(p, q), (what, k)
    if optimizer_state:
        s1, s2 = o1.state_dict()["state"], o2.state_dict()["state"]
        assert s1.keys() == s2.keys() and len(s1) > 100, what
        for i in s1:
            assert tensors_equal(s1[i], s2[i]), (what, i)
    assert e1.updates == e2.updates
    assert tensors_equal(e1.ema.state_dict(), e2.ema.state_dict()), what


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_train_step_equals_the_eager_loop(A, kind, dtype):
    from asy_vrnet_amd import losses, optim
    from asy_vrnet_amd.graph import TrainStep
    eager, captured = trainer(A, kind, dtype), trainer(A, kind, dtype)
    _, m, yl, opt, ema = eager
    w = torch.ones(NS, device="cuda")
    step = TrainStep(captured[1], captured[2], captured[3], captured[4], B, S, NS, max_gt=64)
    assert len(step.graphs) == 1
    trainers_equal(eager, captured, "after construction", optimizer_state=False)      # the warm-up left no trace
    p0 = m.head.stems[0].conv.weight.detach().clone()
    for it in range(4):
        if it == 2:                                                              # a baked-in lr would miss this
            for o in (opt, captured[3]):
                optim.set_optimizer_lr(o, lambda epoch: 3.1e-3 if kind == "sgd" else 4e-4, 0)
        x, r, labels, pngs, seg_labels = batch_of(A, 40 + it)
        opt.zero_grad()
        det, seg = m(x, r)
        total, ldet, lseg = losses.training_loss(yl, det, seg, labels, pngs.cuda(), seg_labels.cuda(), w, NS, True, True)
        total.backward()
        opt.step()
        ema.update(m)
        res = step(x, r, labels, pngs, seg_labels)
        assert torch.isfinite(total)
        assert torch.equal(res["total"], total.detach()), (it, float(res["total"]), float(total))
        assert torch.equal(res["loss_det"], ldet.detach()) and torch.equal(res["loss_seg"], lseg.detach()), it
        trainers_equal(eager, captured, f"step {it}")
    assert ema.updates == 4 and not torch.equal(m.head.stems[0].conv.weight, p0)


def test_an_eager_step_in_between_and_a_checkpoint_keep_working(A):
    """State sharing: an eager step (odd last batch) between two captured ones takes the .grad tensors and the table's
    gradient row; the next captured step takes them back.  And a checkpoint of the optimizer loads into a fresh one."""
    from asy_vrnet_amd import losses, optim
    from asy_vrnet_amd.graph import TrainStep
    eager, captured = trainer(A, "adam"), trainer(A, "adam")
    w = torch.ones(NS, device="cuda")
    step = TrainStep(captured[1], captured[2], captured[3], captured[4], B, S, NS, max_gt=8)

    def eager_step(t, batch):
        _, m, yl, opt, ema = t
        x, r, labels, pngs, seg_labels = batch
        opt.zero_grad()
        det, seg = m(x, r)
        total = losses.training_loss(yl, det, seg, labels, pngs.cuda(), seg_labels.cuda(), w, NS, True, True)[0]
        total.backward()
        opt.step()
        ema.update(m)
        return total.detach()
    for it, mode in enumerate(("captured", "eager", "captured", "captured")):
        batch = batch_of(A, 30 + it)
        total = eager_step(eager, batch)
        got = step(*batch)["total"] if mode == "captured" else eager_step(captured, batch)
        assert torch.equal(got, total), (it, mode)
        trainers_equal(eager, captured, f"step {it} ({mode})")
    sd = captured[3].state_dict()
    assert {int(st["step"]) for st in sd["state"].values()} == {4}
    fresh = optim.build_optimizer(captured[1], "adam", 1e-3, 0.937, 5e-4)
    fresh.load_state_dict(sd)
    assert tensors_equal(fresh.state_dict()["state"][0], eager[3].state_dict()["state"][0])


# ---- 4. / 7. bytes in, and host validation -----------------------------------------------------------------------------
def bytes_of(seed):
    rng = np.random.default_rng(seed)
    img = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8))
    lab = np.kron(rng.integers(0, NS + 1, (B, S // 8, S // 8)), np.ones((8, 8), dtype=np.int64)).astype(np.uint8)
    return img, torch.from_numpy(lab)


@pytest.fixture(scope="module")
def pair(A):
    """Two identical trainers under a TrainStep each: float inputs and bytes."""
    from asy_vrnet_amd.graph import TrainStep
    out = []
    for from_bytes in (False, True):
        t = trainer(A, "sgd")
        out.append((t, TrainStep(t[1], t[2], t[3], t[4], B, S, NS, max_gt=8, from_bytes=from_bytes, f_score=True)))
    return out


def test_from_bytes_equals_the_float_inputs(A, pair):
    from asy_vrnet_amd import data
    (tf, step_f), (tb, step_b) = pair
    for it in range(2):
        _, r, labels, _, _ = batch_of(A, 60 + it)
        img, lab = bytes_of(70 + it)
        images, png, onehot = data.device_batch(img, lab, NS)
        rf = step_f(images, r, labels, png, onehot)
        rb = step_b(img, r, labels, lab)
        assert rf.keys() == rb.keys() == {"total", "loss_det", "loss_seg", "f_score"}
        assert all(torch.equal(rf[k], rb[k]) for k in rf), it
        assert torch.equal(step_b.x, images) and torch.equal(step_b.png, png) and torch.equal(step_b.onehot, onehot)
        trainers_equal(tf, tb, f"step {it}")


def test_host_validation_raises_before_any_launch(A, pair):
    (tf, step_f), (tb, step_b) = pair
    x, r, labels, pngs, seg_labels = batch_of(A, 80)
    img, lab = bytes_of(81)

    def snapshot(t):
        _, m, _, opt, ema = t
        return ([p.detach().clone() for p in m.parameters()] + [b.clone() for b in m.buffers()] +
                [v.clone() for st in opt.state_dict()["state"].values() for v in st.values() if torch.is_tensor(v)] +
                [v.clone() for v in ema.ema.state_dict().values()], ema.updates)
    before = snapshot(tf), snapshot(tb), step_f.stats(), step_b.stats()
    launches = [A.hip.kernel_launches(f) for f in range(1, 14)]
    too_many = [labels[0], torch.ones(9, 5)]
    with pytest.raises(RuntimeError, match="image 1"):
        step_f(x, r, too_many, pngs, seg_labels)                                  # n_1 = 9 > max_gt = 8
    with pytest.raises(RuntimeError, match="shape"):
        step_f(torch.cat([x, x]), torch.cat([r, r]), labels + labels, torch.cat([pngs, pngs]),
               torch.cat([seg_labels, seg_labels]))                               # wrong batch
    with pytest.raises(RuntimeError, match="target lists"):
        step_f(x, r, labels[:1], pngs, seg_labels)
    with pytest.raises(RuntimeError, match="uint8"):
        step_b(x, r, labels, lab)                                                 # float images with from_bytes=True
    with pytest.raises(RuntimeError, match="one-hot"):
        step_f(x, r, labels, pngs)                                                # dice loss without one-hot labels
    torch.cuda.synchronize()
    assert launches == [A.hip.kernel_launches(f) for f in range(1, 14)]
    after = snapshot(tf), snapshot(tb), step_f.stats(), step_b.stats()
    for (ta, ua), (tb_, ub) in zip(before[:2], after[:2]):
        assert ua == ub and all(torch.equal(p, q) for p, q in zip(ta, tb_))
    assert before[2]["steps"] == after[2]["steps"] and before[3]["steps"] == after[3]["steps"]


def test_construction_rejects_groups_with_different_lr(A):
    from asy_vrnet_amd.graph import TrainStep
    _, m, yl, opt, ema = trainer(A, "sgd")
    opt.param_groups[1]["lr"] = 0.5
    with pytest.raises(RuntimeError, match="lr"):
        TrainStep(m, yl, opt, ema, B, S, NS)


# ---- 5. epoch statistics ------------------------------------------------------------------------------------------------
def test_stats_are_the_fp64_means_with_one_read_back(A):
    from asy_vrnet_amd.graph import TrainStep
    _, m, yl, opt, _ = trainer(A, "sgd")
    step = TrainStep(m, yl, opt, None, B, S, NS, max_gt=8, f_score=True)           # ema=None: no EMA in the update graph
    assert step.stats()["steps"] == 0
    seen = []
    for it in range(4):
        x, r, labels, pngs, seg_labels = batch_of(A, 90 + it)
        res = step(x, r, labels, pngs, seg_labels)
        seen.append({k: v.clone() for k, v in res.items()})                        # valid until the next call
    st = step.stats()
    assert st["steps"] == 4 and set(st) == {"steps", "total", "loss_det", "loss_seg", "f_score"}
    for k in seen[0]:
        vals = [float(s[k].double()) for s in seen]
        assert st[k] == sum(vals) / 4, k
    assert 0.0 <= st["f_score"] <= 1.0 and len({float(s["total"]) for s in seen}) == 4
    step.reset_stats()
    x, r, labels, pngs, seg_labels = batch_of(A, 95)
    res = step(x, r, labels, pngs, seg_labels)
    st = step.stats()
    assert st["steps"] == 1 and all(st[k] == float(res[k].double()) for k in res)


# ---- 6. one RCCL rank ---------------------------------------------------------------------------------------------------
def test_data_parallel_single_rank_equals_the_plain_step(A):
    import torch.distributed as dist
    from asy_vrnet_amd.graph import TrainStep
    from asy_vrnet_amd.parallel import DataParallelVRNet
    own_group = not dist.is_initialized()
    if own_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29593")
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        plain = trainer(A, "sgd")
        wrapped = trainer(A, "sgd", net_of=lambda m: DataParallelVRNet(m, force_collective=True))
        step_p = TrainStep(plain[0], plain[2], plain[3], plain[4], B, S, NS, max_gt=8)
        step_w = TrainStep(wrapped[0], wrapped[2], wrapped[3], wrapped[4], B, S, NS, max_gt=8)
        assert len(step_p.graphs) == 1 and len(step_w.graphs) == 3
        for it in range(2):
            x, r, labels, pngs, seg_labels = batch_of(A, 50 + it)
            rp = step_p(x, r, labels, pngs, seg_labels)
            rw = step_w(x, r, labels, pngs, seg_labels)
            assert all(torch.equal(rp[k], rw[k]) for k in rp), it
            trainers_equal(plain, wrapped, f"step {it}")
    finally:
        if own_group:
            dist.destroy_process_group()
