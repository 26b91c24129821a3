"""CPU: the fused Adam kernels (csrc/adam_kernels.h) on the emulation build, optim.FlatAdam on top of them, checkpoints in
torch.optim.Adam's format, and the entries' argument validation on the product library.  tests/adam_cases.py has the cases."""
import ctypes as C
import os

import pytest
import torch

import adam_cases as AC
from emul_util import emul_lib  # noqa: F401

CPU = torch.device("cpu")


def _flat_cases():
    # sizes are expressed through the library's limits at run time: index into adam_cases.flat_sizes()
    cases = [(i, 0.0, 1.0) for i in range(8)]
    return cases + [(7, 1e-2, 1.0), (7, 0.0, 0.125), (7, 1e-2, 0.125), (6, 1e-2, 0.125)]


def test_limits(emul_lib):
    c, s = AC.limits()
    assert c >= 256 and c % 4 == 0 and s >= 67            # MVSNet (55 tensors, 67 with the refine net) and CVP-MVSNet (50) fit in one launch
    assert s * 16 + 256 < 4096                               # the argument block stays well under 4 KB


@pytest.mark.parametrize("size_index,wd,scale", _flat_cases())
def test_flat_accuracy(emul_lib, size_index, wd, scale):
    AC.check_flat_accuracy(CPU, AC.flat_sizes()[size_index], wd, scale)


@pytest.mark.parametrize("leads", [(1, 1, 1), (3, 3, 3), (0, 1, 2), (4, 4, 5)])
def test_flat_accuracy_at_other_alignments(emul_lib, leads):
    """p, m and v start 4, 12 bytes behind a 16-byte boundary (vector path with a scalar head) or disagree (4-byte path)."""
    AC.check_flat_accuracy(CPU, AC.flat_sizes()[7], 1e-2, 0.125, leads=leads)


@pytest.mark.parametrize("kind", ["lengths", "null", "many", "many+1", "view"])
@pytest.mark.parametrize("leads,wd,scale", [((4, 4, 4), 0.0, 1.0), ((1, 1, 1), 1e-2, 0.125), ((0, 3, 2), 1e-2, 1.0)])
def test_table_path_equals_flat_path(emul_lib, kind, leads, wd, scale):
    AC.check_table_equals_flat(CPU, kind, leads=leads, wd=wd, grad_scale=scale)


def test_uncovered_elements_untouched(emul_lib):
    AC.check_uncovered_elements_untouched(CPU)


def test_exact_properties(emul_lib):
    AC.check_exact_properties(CPU)


def test_flat_adam_against_stock_adam_small_model(emul_lib):
    AC.check_flat_adam_on_model(CPU, AC.small_model(), "small model")


def test_flat_adam_against_stock_adam_mvsnet(emul_lib):
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(0)
    AC.check_flat_adam_on_model(CPU, MVSNet(refine=True), "MVSNet(refine=True)")


def test_flat_adam_constructor_rejections(emul_lib):
    from mvs_amd.dist import FlatGradBucket
    from mvs_amd.optim import FlatAdam
    net = AC.small_model()
    with pytest.raises(ValueError, match="one parameter group"):
        FlatAdam([{"params": list(net[0].parameters())}, {"params": list(net[2].parameters())}])
    with pytest.raises(ValueError, match="amsgrad"):
        FlatAdam(net.parameters(), amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        FlatAdam(net.parameters(), maximize=True)
    with pytest.raises(ValueError, match="flatten_params=True"):
        FlatAdam(net.parameters(), bucket=FlatGradBucket(net.parameters()))
    with pytest.raises(ValueError, match="betas"):
        FlatAdam(net.parameters(), betas=(0.9, 1.0))
    bucket = FlatGradBucket(net.parameters(), flatten_params=True)
    opt = FlatAdam(net.parameters(), bucket=bucket)
    assert opt.bucket is bucket
    with pytest.raises(ValueError, match="one parameter group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})


def test_missing_gradient_is_a_zero_gradient(emul_lib):
    """A parameter without a .grad is updated with zeros (gather()'s meaning): null pointer on the table path."""
    from mvs_amd.optim import FlatAdam
    nets = [AC.small_model(), AC.small_model()]
    opts = [FlatAdam(n.parameters(), weight_decay=1e-2) for n in nets]
    for net, opt, drop in zip(nets, opts, (True, False)):
        params = list(net.parameters())
        gs = AC.model_grads(params, 1)[0]
        gs[1] = torch.zeros_like(gs[1])
        AC.assign_grads(params, gs)
        if drop:
            params[1].grad = None
        emul_lib.launch_trace()
        opt.step()
        assert emul_lib.launch_trace() == ["adam_table"]
    AC.assert_bits_equal((opts[0].bucket.flat_param.data, opts[0].exp_avg, opts[0].exp_avg_sq),
                         (opts[1].bucket.flat_param.data, opts[1].exp_avg, opts[1].exp_avg_sq), "missing against zero gradient")


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------
def _stock(net, wd=1e-2):
    return torch.optim.Adam(net.parameters(), lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=wd, foreach=False)


def _truth_after(params0, grads, wd=1e-2):
    (tp, tm, tv), _, _ = AC.stock_and_truth(params0, grads, [AC.LR] * len(grads), wd=wd)
    return AC.flat_cat(tp), AC.flat_cat(tm), AC.flat_cat(tv)


def _stock_tensors(opt, params):
    return (AC.flat_cat(params), AC.flat_cat([opt.state[p]["exp_avg"] for p in params]),
            AC.flat_cat([opt.state[p]["exp_avg_sq"] for p in params]))


def _flat_tensors(opt, params):
    sd = opt.state_dict()["state"]
    return (AC.flat_cat(params), AC.flat_cat([sd[k]["exp_avg"] for k in range(len(params))]),
            AC.flat_cat([sd[k]["exp_avg_sq"] for k in range(len(params))]))


def test_checkpoint_from_stock_adam_resumes_in_flat_adam(emul_lib):
    from mvs_amd.optim import FlatAdam
    net_s, net_f, net_y = AC.small_model(), AC.small_model(), AC.small_model()
    ps, pf, py = list(net_s.parameters()), list(net_f.parameters()), list(net_y.parameters())
    params0 = [p.detach().clone() for p in ps]
    grads = AC.model_grads(ps, 5)
    stock = _stock(net_s)
    for gs in grads[:3]:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        stock.step()
    ckpt_model, ckpt_opt = {k: v.clone() for k, v in net_s.state_dict().items()}, stock.state_dict()
    net_f.load_state_dict(ckpt_model)
    flat = FlatAdam(net_f.parameters(), lr=0.5, weight_decay=0.0)          # the checkpoint's hyper-parameters replace these
    flat.load_state_dict(ckpt_opt)
    assert flat.steps_taken() == 3 and flat.param_groups[0]["lr"] == AC.LR and flat.param_groups[0]["weight_decay"] == 1e-2
    net_y.load_state_dict(ckpt_model)
    yard = _stock(net_y)
    yard.load_state_dict(ckpt_opt)
    for gs in grads[3:]:
        AC.assign_grads(pf, gs)
        flat.step()
        for p, g in zip(py, gs):
            p.grad = g.clone()
        yard.step()
    assert flat.steps_taken() == 5
    AC.assert_accurate("checkpoint stock -> FlatAdam", CPU, _flat_tensors(flat, pf), _stock_tensors(yard, py), _truth_after(params0, grads))


def test_checkpoint_from_flat_adam_resumes_in_stock_adam(emul_lib):
    from mvs_amd.optim import FlatAdam
    net_f, net_s, net_y = AC.small_model(), AC.small_model(), AC.small_model()
    pf, ps, py = list(net_f.parameters()), list(net_s.parameters()), list(net_y.parameters())
    params0 = [p.detach().clone() for p in pf]
    grads = AC.model_grads(pf, 5)
    flat = FlatAdam(net_f.parameters(), lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=1e-2)
    for gs in grads[:3]:
        AC.assign_grads(pf, gs)
        flat.step()
    ckpt_model, ckpt_opt = {k: v.clone() for k, v in net_f.state_dict().items()}, flat.state_dict()
    # the yardstick: stock Adam on the whole sequence
    yard = _stock(net_y)
    for gs in grads:
        for p, g in zip(py, gs):
            p.grad = g.clone()
        yard.step()
    net_s.load_state_dict(ckpt_model)
    stock = _stock(net_s, wd=0.0)
    stock.load_state_dict(ckpt_opt)
    assert stock.param_groups[0]["weight_decay"] == 1e-2
    for gs in grads[3:]:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        stock.step()
    assert all(float(stock.state[p]["step"]) == 5.0 for p in ps)
    AC.assert_accurate("checkpoint FlatAdam -> stock", CPU, _stock_tensors(stock, ps), _stock_tensors(yard, py), _truth_after(params0, grads))


def test_state_dict_has_stock_adams_keys_and_shapes(emul_lib):
    from mvs_amd.optim import FlatAdam
    net_f, net_s = AC.small_model(), AC.small_model()
    pf, ps = list(net_f.parameters()), list(net_s.parameters())
    flat, stock = FlatAdam(net_f.parameters(), lr=AC.LR, weight_decay=1e-2), _stock(net_s)
    assert flat.state_dict()["state"] == {} and stock.state_dict()["state"] == {}
    gs = AC.model_grads(pf, 1)[0]
    p0 = [p.detach().clone() for p in pf]
    AC.assign_grads(pf, gs)
    flat.step()
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    stock.step()
    a, b = flat.state_dict(), stock.state_dict()
    assert set(a) == set(b) and len(a["param_groups"]) == 1
    assert set(a["param_groups"][0]) == set(b["param_groups"][0]) and a["param_groups"][0]["params"] == b["param_groups"][0]["params"]
    assert set(a["state"]) == set(b["state"])
    for k in b["state"]:
        assert set(a["state"][k]) == set(b["state"][k])
        for key in ("exp_avg", "exp_avg_sq"):
            assert a["state"][k][key].shape == b["state"][k][key].shape == pf[k].shape
            assert a["state"][k][key].stride() == b["state"][k][key].stride()
        assert float(a["state"][k]["step"]) == float(b["state"][k]["step"]) == 1.0
    # the channels-last parameter's state comes back in its logical shape: element by element (1 - beta1) (g + wd p0) after one step
    k = [i for i, p in enumerate(pf) if p.dim() == 4 and not p.is_contiguous()][0]
    assert torch.allclose(a["state"][k]["exp_avg"], b["state"][k]["exp_avg"], rtol=1e-6, atol=1e-12)
    assert torch.allclose(a["state"][k]["exp_avg"], 0.1 * (gs[k] + 1e-2 * p0[k]), rtol=1e-5, atol=1e-9)


def test_load_rejects_parameters_at_different_steps(emul_lib):
    from mvs_amd.optim import FlatAdam
    net = AC.small_model()
    flat = FlatAdam(net.parameters())
    AC.assign_grads(list(net.parameters()), AC.model_grads(list(net.parameters()), 1)[0])
    flat.step()
    sd = flat.state_dict()
    sd["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="different steps"):
        flat.load_state_dict(sd)
    assert flat.steps_taken() == 1


# ---- argument validation on the product library, no GPU ----------------------------------------------------------------------------
def test_argument_validation_on_the_product_library():
    """Every rejection happens on the host before any launch: ValueError from the wrapper, mvs_last_error() set, no launch label."""
    from mvs_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.MvsLib()
    P = 4096                                                  # a non-null "device pointer": nothing dereferences it before the checks
    ok = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, gs=1.0)

    def flat(p=P, g=P, m=P, v=P, n=8, ctr=P, **kw):
        h = dict(ok, **kw)
        lib.call("mvs_adam_step", p, g, m, v, n, ctr, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["gs"], None)

    def table(p=P, m=P, v=P, n=64, grads=(P, P), offsets=(0, 8), counts=(8, 8), ctr=P, null_arrays=False, **kw):
        h = dict(ok, **kw)
        k = len(grads)
        ga = (C.c_void_p * max(k, 1))(*grads)
        oa, ca = (C.c_longlong * max(k, 1))(*offsets), (C.c_longlong * max(k, 1))(*counts)
        lib.call("mvs_adam_step_table", p, m, v, n, None if null_arrays else ga, oa, ca, k, ctr, h["lr"], h["b1"], h["b2"], h["eps"],
                 h["wd"], h["gs"], None)

    nan, inf = float("nan"), float("inf")
    bad_hyper = [dict(lr=-1e-3), dict(b1=-0.1), dict(b1=1.0), dict(b2=1.0), dict(b2=-1e-9), dict(eps=-1e-8), dict(lr=nan), dict(lr=inf),
                 dict(b1=nan), dict(b2=nan), dict(eps=inf), dict(wd=nan), dict(gs=inf), dict(gs=nan)]
    rejected = [(flat, dict(p=None)), (flat, dict(g=None)), (flat, dict(m=None)), (flat, dict(v=None)), (flat, dict(ctr=None)),
                (flat, dict(n=0)), (flat, dict(n=-5)),
                (table, dict(p=None)), (table, dict(m=None)), (table, dict(v=None)), (table, dict(ctr=None)), (table, dict(null_arrays=True)),
                (table, dict(n=0)), (table, dict(grads=(), offsets=(), counts=())),
                (table, dict(offsets=(0, 4))),                               # overlap
                (table, dict(offsets=(8, 0))),                               # unsorted
                (table, dict(offsets=(0, 60))),                              # past n
                (table, dict(offsets=(-1, 8))),                              # in front of 0
                (table, dict(counts=(8, 0)))]                                # empty segment
    rejected += [(fn, h) for h in bad_hyper for fn in (flat, table)]
    lib.launch_trace()
    for fn, kw in rejected:
        with pytest.raises(ValueError):
            fn(**kw)
        assert lib.raw("mvs_last_error"), (fn.__name__, kw)
    assert lib.launch_trace() == []
    with pytest.raises(ValueError, match="null pointer"):
        lib.call("mvs_adam_limits", None, None)
    chunk, segs = C.c_int(), C.c_int()
    lib.call("mvs_adam_limits", C.byref(chunk), C.byref(segs))
    assert chunk.value > 0 and segs.value > 0


def test_cpu_tensors_are_rejected_by_the_product():
    from mvs_amd import _lib, ops
    from mvs_amd.optim import FlatAdam
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    _lib._INSTANCE = None
    z = torch.zeros(8)
    ctr = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_step(z, z.clone(), z.clone(), z.clone(), ctr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_step_table(z, [z.clone()], [0], [8], z.clone(), z.clone(), ctr)
    net = AC.small_model()
    opt = FlatAdam(net.parameters())
    AC.assign_grads(list(net.parameters()), AC.model_grads(list(net.parameters()), 1)[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
