"""Shared cases of the fused Adam tests (tests/test_adam.py on the CPU emulation, tests/test_gpu_adam.py on the GPU): the fp64
restatement of the update, seeded problems, and the checks themselves as functions of the device.

Criterion of the accuracy checks: truth is the fp64 restatement below, the yardstick is torch.optim.Adam(foreach=False) in fp32 on the
CPU on the same sequence; conftest.assert_as_accurate_as_fp32_reference with slack = 4 and floor = one fp32 ulp of the tensor's largest
magnitude (2**-23 * max|t|: derived from the number format, not measured).  A CPU probe of the plain fp32 chain with the constants
formed in fp64 stays within 2.7x of the yardstick's error; forming 1 - beta2 in fp32 is 30x off on exp_avg_sq, which slack = 4 catches."""
import json
import os

import torch

from conftest import assert_as_accurate_as_fp32_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 12345.0
BETAS = (0.9, 0.999)
EPS = 1e-8
LR = 1e-3


def limits():
    from mvs_amd import ops
    return ops.adam_limits()


def flat_sizes():
    c, _ = limits()
    return [1, 3, 4, 5, c - 1, c, c + 1, 3 * c + 7]


def table_lengths():
    c, _ = limits()
    return [1, 3, 8, 216, 1, c - 1, c, c + 1, 2 * c + 5, 5]


# ---- the truth ---------------------------------------------------------------------------------------------------------------------
def adam_truth64(p, m, v, grad, t, lr=LR, betas=BETAS, eps=EPS, wd=0.0, grad_scale=1.0):
    """One step of torch.optim.Adam's formulas in fp64 (L2 weight decay), t = 1, 2, ...  Returns the new (p, m, v)."""
    b1, b2 = betas
    g = grad.double() * grad_scale
    if wd != 0:
        g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v


def problem(n, steps=20, seed=0):
    """Seeded parameters with a block 1e-4 times smaller than the rest, and `steps` gradients whose per-step magnitude spans 1e-6 .. 1
    with 10 % exact zeros."""
    gen = torch.Generator().manual_seed(1000 + seed)
    p0 = torch.randn(n, generator=gen)
    p0[n // 3: n // 3 + max(1, n // 4)] *= 1e-4
    grads = []
    for s in range(steps):
        mag = 10.0 ** (-6.0 * s / max(1, steps - 1))                 # 1 .. 1e-6
        g = torch.randn(n, generator=gen) * mag
        g[torch.rand(n, generator=gen) < 0.1] = 0.0
        grads.append(g)
    return p0, grads


def reference_runs(p0, grads, lr=LR, wd=0.0, grad_scale=1.0, lrs=None):
    """(truth64, stock32): each (p, exp_avg, exp_avg_sq) after the whole sequence.  lrs: a learning rate per step (a schedule)."""
    p, m, v = p0.double(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    for s, g in enumerate(grads):
        step_lr = lrs[s] if lrs is not None else lr
        p, m, v = adam_truth64(p, m, v, g, s + 1, lr=step_lr, wd=wd, grad_scale=grad_scale)
        opt.param_groups[0]["lr"] = step_lr
        q.grad = g * grad_scale                                       # fp32; exact for the power-of-two scales of the cases
        opt.step()
    st = opt.state[q]
    return (p, m, v), (q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())


def record_ratios(what, dev, names, ours, ref32, truth64):
    """Measured error ratios of one accuracy check, printed, and appended to the file MVS_ADAM_REPORT names when it is set;
    profiles/adam_parity_ratios.jsonl is such a file from a run of tests/test_gpu_adam.py, kept with the repository."""
    out = os.environ.get("MVS_ADAM_REPORT", "")
    row = {"what": what, "device": str(dev), "slack_allowed": 4.0}
    for name, o, r, t in zip(names, ours, ref32, truth64):
        e_o, e_r = (o.double() - t).abs(), (r.double() - t).abs()
        row[name] = {"max_err": float(e_o.max()), "ref_max_err": float(e_r.max()), "mean_err": float(e_o.mean()),
                     "ref_mean_err": float(e_r.mean()), "floor": 2.0 ** -23 * float(t.abs().max()),
                     "max_ratio": float(e_o.max()) / max(float(e_r.max()), 1e-300),
                     "mean_ratio": float(e_o.mean()) / max(float(e_r.mean()), 1e-300)}
    print("adam parity", json.dumps(row))
    if out:
        try:
            with open(out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        except OSError:
            pass


def assert_accurate(what, dev, ours, ref32, truth64):
    names = ("p", "exp_avg", "exp_avg_sq")
    ours = [o.detach().cpu() for o in ours]
    record_ratios(what, dev, names, ours, ref32, truth64)
    for name, o, r, t in zip(names, ours, ref32, truth64):
        assert_as_accurate_as_fp32_reference(o, r, t, slack=4.0, floor=2.0 ** -23 * float(t.abs().max()), what="%s %s" % (what, name))


# ---- state with canaries -------------------------------------------------------------------------------------------------------------
class State:
    """p, m, v as slices of larger buffers with canary values in front and behind (`leads`: canary elements in front of each, which
    also sets the three addresses mod 16), and the int32 [2] counter."""

    def __init__(self, p0, dev, leads=(4, 4, 4), tail=5):
        n = p0.numel()
        self.n, self.bufs, self.leads = n, [], leads
        for lead, init in zip(leads, (p0, torch.zeros(n), torch.zeros(n))):
            buf = torch.full((lead + n + tail,), CANARY, dtype=torch.float32, device=dev)
            buf[lead:lead + n] = init.to(dev)
            self.bufs.append(buf)
        self.p, self.m, self.v = (b[lead:lead + n] for b, lead in zip(self.bufs, leads))
        self.counter = torch.zeros(2, dtype=torch.int32, device=dev)

    def assert_canaries(self):
        for b, lead in zip(self.bufs, self.leads):
            assert bool((b[:lead] == CANARY).all()) and bool((b[lead + self.n:] == CANARY).all()), "a canary was overwritten"

    def tensors(self):
        return self.p.clone(), self.m.clone(), self.v.clone()


def assert_bits_equal(a, b, what):
    for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s: %s differs in %d elements" % (
            what, name, int((x.view(torch.int32) != y.view(torch.int32)).sum()))


def run_flat(state, grads, dev, lr=LR, wd=0.0, grad_scale=1.0):
    from mvs_amd import ops
    for s, g in enumerate(grads):
        gd = g.to(dev)
        keep = gd.clone()
        ops.adam_step(state.p, gd, state.m, state.v, state.counter, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, grad_scale=grad_scale)
        assert torch.equal(gd.view(torch.int32), keep.view(torch.int32)), "the gradient was modified"
        assert state.counter.tolist() == [s + 1, 0], "counter %s after step %d" % (state.counter.tolist(), s + 1)
    state.assert_canaries()


# ---- checks, as functions of the device ------------------------------------------------------------------------------------------------
def check_flat_accuracy(dev, n, wd, grad_scale, leads=(4, 4, 4)):
    p0, grads = problem(n, seed=n)
    state = State(p0, dev, leads)
    run_flat(state, grads, dev, wd=wd, grad_scale=grad_scale)
    truth, stock = reference_runs(p0, grads, wd=wd, grad_scale=grad_scale)
    assert_accurate("flat n=%d wd=%g scale=%g leads=%s" % (n, wd, grad_scale, leads), dev, state.tensors(), stock, truth)


def make_table(kind, dev, steps, seed=3):
    """(n, offsets, counts, per-step gradient lists with None for a null pointer, per-step packed gradients [n]).  Gradients are
    allocated separately; kind 'view' passes one as a view at a 4-byte offset into a larger tensor."""
    c, s = limits()
    if kind == "many":
        lengths = [1] * s
    elif kind == "many+1":
        lengths = [1] * (s + 1)
    else:
        lengths = table_lengths()
    offsets, off = [], 0
    for ln in lengths:
        offsets.append(off)
        off += ln
    n = off
    null_at = {3, 8} if kind == "null" else set()
    gen = torch.Generator().manual_seed(seed)
    per_step, packed = [], []
    for st in range(steps):
        gs, flat = [], torch.zeros(n)
        for k, (o, ln) in enumerate(zip(offsets, lengths)):
            if k in null_at:
                gs.append(None)
                continue
            g = torch.randn(ln, generator=gen) * 10.0 ** (-st)
            g[torch.rand(ln, generator=gen) < 0.1] = 0.0
            flat[o:o + ln] = g
            if kind == "view" and k == 8:
                big = torch.zeros(ln + 9, device=dev)                 # base 16-byte aligned (the allocator's granularity)
                big[1:1 + ln] = g.to(dev)
                gd = big[1:1 + ln]
                assert gd.data_ptr() % 16 == 4
            else:
                gd = g.to(dev).clone()
            gs.append(gd)
        per_step.append(gs)
        packed.append(flat)
    return n, offsets, lengths, per_step, packed


def check_table_equals_flat(dev, kind, leads=(4, 4, 4), wd=0.0, grad_scale=1.0, steps=3):
    from mvs_amd import _lib, ops
    lib = _lib.get()
    _, smax = limits()
    n, offsets, counts, per_step, packed = make_table(kind, dev, steps)
    p0, _ = problem(n, steps=0, seed=7)
    a, b = State(p0, dev, leads), State(p0, dev, leads)
    run_flat(a, packed, dev, wd=wd, grad_scale=grad_scale)
    for s, gs in enumerate(per_step):
        keep = [None if g is None else g.clone() for g in gs]
        lib.launch_trace()
        ops.adam_step_table(b.p, gs, offsets, counts, b.m, b.v, b.counter, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd,
                            grad_scale=grad_scale)
        want = ["adam_table part"] * ((len(gs) - 1) // smax) + ["adam_table"]
        assert lib.launch_trace() == want
        assert b.counter.tolist() == [s + 1, 0], "counter %s after step %d" % (b.counter.tolist(), s + 1)
        for g, k in zip(gs, keep):
            assert g is None or torch.equal(g.view(torch.int32), k.view(torch.int32)), "a gradient was modified"
    b.assert_canaries()
    assert_bits_equal(a.tensors(), b.tensors(), "table '%s' against the flat path" % kind)
    assert a.counter.tolist() == b.counter.tolist()


def check_uncovered_elements_untouched(dev):
    """A table that covers only part of [0, n): the rest keeps its bits, state included."""
    from mvs_amd import ops
    c, _ = limits()
    n = 2 * c + 9
    p0, grads = problem(n, steps=1, seed=11)
    st = State(p0, dev)
    segs = [(2, 5), (c - 3, 7), (2 * c + 1, 3)]
    gs = [grads[0][o:o + ln].to(dev).clone() for o, ln in segs]
    ops.adam_step_table(st.p, gs, [o for o, _ in segs], [ln for _, ln in segs], st.m, st.v, st.counter)
    covered = torch.zeros(n, dtype=torch.bool)
    for o, ln in segs:
        covered[o:o + ln] = True
    p = st.p.cpu()
    assert torch.equal(p[~covered].view(torch.int32), p0[~covered].view(torch.int32))
    assert bool((st.m.cpu()[~covered] == 0).all()) and bool((st.v.cpu()[~covered] == 0).all())
    assert bool((p[covered] != p0[covered]).any()) and st.counter.tolist() == [1, 0]
    st.assert_canaries()


def check_exact_properties(dev):
    from mvs_amd import ops
    c, _ = limits()
    n = c + 37
    p0, grads = problem(n, steps=2, seed=5)
    # (a) wd = 0, zero gradient and zero state: the parameter keeps its bits
    g0 = grads[0].clone()
    g0[::3] = 0.0
    st = State(p0, dev, leads=(1, 1, 1))
    run_flat(st, [g0], dev)
    p = st.p.cpu()
    assert torch.equal(p[::3].view(torch.int32), p0[::3].view(torch.int32))
    assert bool((st.m.cpu()[::3] == 0).all()) and bool((st.v.cpu()[::3] == 0).all())
    # (b) a NaN / Inf gradient element changes only its own element
    bad = grads[0].clone()
    where = [0, 5, c - 1, c, n - 1]
    for j, i in enumerate(where):
        bad[i] = (float("nan"), float("inf"), float("-inf"))[j % 3]
    clean, dirty = State(p0, dev), State(p0, dev)
    run_flat(clean, [grads[0]], dev)
    run_flat(dirty, [bad], dev)
    keep = torch.ones(n, dtype=torch.bool)
    keep[where] = False
    for x, y in zip(clean.tensors(), dirty.tensors()):
        assert torch.equal(x.cpu()[keep].view(torch.int32), y.cpu()[keep].view(torch.int32))
    assert not bool(torch.isfinite(dirty.p.cpu()[where]).any())
    # (c) two runs from the same state are bit-identical
    r1, r2 = State(p0, dev), State(p0, dev)
    run_flat(r1, grads, dev, wd=1e-2)
    run_flat(r2, grads, dev, wd=1e-2)
    assert_bits_equal(r1.tensors(), r2.tensors(), "two runs")


# ---- FlatAdam on a model ---------------------------------------------------------------------------------------------------------------
def small_model(seed=0):
    """A few tensors of odd sizes, one of them channels-last."""
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.Conv2d(5, 7, 3, bias=False),
                              torch.nn.Conv2d(7, 1, 1))
    net[2].weight.data = net[2].weight.data.contiguous(memory_format=torch.channels_last)
    return net


def model_grads(params, steps, seed=0):
    """Seeded synthetic gradients, per step a list in the parameters' logical shapes (CPU)."""
    gen = torch.Generator().manual_seed(500 + seed)
    out = []
    for s in range(steps):
        out.append([torch.randn(p.shape, generator=gen) * 10.0 ** (-s) * (torch.rand(p.shape, generator=gen) >= 0.1) for p in params])
    return out


def assign_grads(params, grads):
    """.grad tensors as autograd leaves them: freshly allocated, laid out with the parameter's strides."""
    for p, g in zip(params, grads):
        p.grad = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device).copy_(g)


def stock_and_truth(params0, grads, lrs, wd=0.0, t0_state=None):
    """Stock fp32 Adam (CPU, foreach=False) and the fp64 truth over per-parameter tensors.  params0: CPU tensors.  Returns
    (truth (p, m, v) lists, stock optimiser, stock parameters)."""
    qs = [torch.nn.Parameter(p.clone()) for p in params0]
    opt = torch.optim.Adam(qs, lr=lrs[0], betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    tp = [p.double() for p in params0]
    tm, tv = [torch.zeros_like(p) for p in tp], [torch.zeros_like(p) for p in tp]
    for s, gs in enumerate(grads):
        opt.param_groups[0]["lr"] = lrs[s]
        for q, g in zip(qs, gs):
            q.grad = g.clone()
        opt.step()
        for k, g in enumerate(gs):
            tp[k], tm[k], tv[k] = adam_truth64(tp[k], tm[k], tv[k], g, s + 1, lr=lrs[s], wd=wd)
    return (tp, tm, tv), opt, qs


def flat_cat(ts):
    return torch.cat([t.detach().cpu().reshape(-1) for t in ts])


def check_flat_adam_on_model(dev, net, what):
    """Five steps with a MultiStepLR milestone inside them against the fp64 truth, stock fp32 Adam as the yardstick; one kernel label
    per step on the table path; a gradient in other strides than its parameter's takes the flat path and gives the same bits."""
    from mvs_amd import _lib
    from mvs_amd.optim import FlatAdam
    lib = _lib.get()
    net = net.to(dev)
    params = [p for p in net.parameters() if p.requires_grad]
    cl = [k for k, p in enumerate(params) if p.dim() == 4 and not p.is_contiguous()]
    assert cl, "the case needs a channels-last parameter"
    params0 = [p.detach().cpu().clone() for p in params]
    steps, wd = 5, 1e-2
    grads = model_grads(params, steps)
    opt = FlatAdam(net.parameters(), lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.1)
    lrs = []
    for s in range(steps):
        opt.zero_grad()
        assert all(p.grad is None for p in params)
        assign_grads(params, grads[s])
        lrs.append(opt.param_groups[0]["lr"])
        lib.launch_trace()
        opt.step()
        assert lib.launch_trace() == ["adam_table"]
        sched.step()
    assert lrs[:2] == [LR, LR] and abs(lrs[2] - 0.1 * LR) < 1e-12 and opt.steps_taken() == steps
    (tp, tm, tv), stock, qs = stock_and_truth(params0, grads, lrs, wd=wd)
    sd = opt.state_dict()
    ours = (flat_cat(params), flat_cat([sd["state"][k]["exp_avg"] for k in range(len(params))]),
            flat_cat([sd["state"][k]["exp_avg_sq"] for k in range(len(params))]))
    ref = (flat_cat(qs), flat_cat([stock.state[q]["exp_avg"] for q in qs]), flat_cat([stock.state[q]["exp_avg_sq"] for q in qs]))
    assert_accurate("FlatAdam %s" % what, dev, ours, ref, (flat_cat(tp), flat_cat(tm), flat_cat(tv)))
    # the same state twice: once more on the table path, once with the channels-last parameter's gradient handed over contiguous
    snap_p, snap_s = opt.bucket.flat_param.data.clone(), opt.state_buffer.clone()
    extra = model_grads(params, 1, seed=9)[0]
    assign_grads(params, extra)
    opt.step()
    table_result = (opt.bucket.flat_param.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    opt.bucket.flat_param.data.copy_(snap_p)
    opt.state_buffer.copy_(snap_s)
    assign_grads(params, extra)
    params[cl[0]].grad = extra[cl[0]].to(dev).contiguous()
    assert params[cl[0]].grad.stride() != params[cl[0]].stride()
    lib.launch_trace()
    opt.step()
    assert lib.launch_trace() == ["adam_flat"]
    assert_bits_equal(table_result, (opt.bucket.flat_param.data, opt.exp_avg, opt.exp_avg_sq), "flat path after a re-laid-out gradient")
    assert opt.steps_taken() == steps + 1
