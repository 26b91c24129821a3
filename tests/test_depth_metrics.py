"""CPU: the seven depth-map validation metrics (csrc/depth_metrics_kernels.h) -- the test-side restatement (tests/metrics_oracle.py)
against the reference's fixture (tests/golden/g16_depth_metrics.npz) and, where the reference tree is present, against its live
import; ops.depth_metrics and every drop-in of both trees through the emulated kernels; the entry point's argument checks against
the product library."""
import ctypes as C
import os

import pytest
import torch

from conftest import load_golden
from emul_util import emul_lib  # noqa: F401
import metrics_oracle as M

torch.set_num_threads(4)
REF = "/root/reference"
T = len(M.THRESHOLDS)


@pytest.fixture(scope="module")
def fixture():
    return load_golden("g16_depth_metrics")


def _ours(est, gt, mask, interval, **kw):
    from mvs_amd import ops
    return ops.depth_metrics(est, gt, mask, interval, M.THRESHOLDS, **kw)


@pytest.mark.parametrize("prefix", M.CASES)
def test_oracle_vs_reference_fixture(fixture, prefix):
    """metrics_oracle's fp32 restatement against what the reference returned, by the metrics' own criteria (bit equality on the
    generating CPU is asserted by the generator; another CPU may order an fp32 sum differently), and its fp64 values against
    the stored truth."""
    est, gt, mask, interval = M.decode_case(fixture, prefix)
    r_out, r_per, t_out, t_per = M.fixture_results(fixture, prefix)
    o32, p32 = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float32)
    M.check_against(o32, p32, r_out, r_per, t_out, t_per, T, what=prefix + "oracle32")
    o64, p64 = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float64)
    assert torch.equal(torch.isnan(o64), torch.isnan(t_out)) and torch.equal(torch.isnan(p64), torch.isnan(t_per))
    assert bool(((torch.nan_to_num(o64) - torch.nan_to_num(t_out)).abs() <= 1e-12 * torch.nan_to_num(t_out).abs()).all())
    assert bool(((torch.nan_to_num(p64) - torch.nan_to_num(t_per)).abs() <= 1e-12 * torch.nan_to_num(t_per).abs()).all())


def test_fixture_cases_are_what_they_claim(fixture):
    """The inputs hold the situations the cases are there for: pixels exactly on every decision value, an empty mask, the two NaN
    positions, a mask that is not [gt != 0], and the NaN pattern each of them produces in the reference."""
    est, gt, mask, interval = M.decode_case(fixture, "c1_")
    d = (est - gt).abs()[1]
    assert interval.tolist() == pytest.approx([2.65, 2.5, 3.0]) and float(interval[1]) == 2.5
    for v in (2.0, 4.0, 8.0, 2.5, 7.5):
        assert int((d == v).sum()) >= 1, v
    assert int(((d == 2) | (d == 4) | (d == 8) | (d == 2.5) | (d == 7.5)).sum()) >= 8
    assert torch.equal(mask, gt > 0) and 0.25 < float((gt == 0).float().mean()) < 0.35
    assert not bool(M.decode_case(fixture, "c3_")[2][2].any())
    e4, g4, m4, _ = M.decode_case(fixture, "c4_")
    assert int(torch.isnan(e4).sum()) == 1 and bool(m4[torch.isnan(e4)].all())
    e5, g5, m5, _ = M.decode_case(fixture, "c5_")
    assert int(torch.isnan(e5).sum()) == 1 and float(g5[torch.isnan(e5)]) == 0.0 and not bool(m5[torch.isnan(e5)].any())
    _, g6, m6, _ = M.decode_case(fixture, "c6_")
    assert int((m6 != (g6 != 0)).sum()) > 500
    nan = lambda p: torch.isnan(fixture[p + "out32"]).tolist()
    assert nan("c1_") == [False] * 7 and nan("c2_") == [False] * 7 and nan("c6_") == [False] * 7
    assert nan("c3_") == [True] * 4 + [False] * 3
    assert nan("c4_") == [True, False, False, False, True, False, False]
    assert nan("c5_") == [False] * 4 + [True, False, False]
    assert tuple(M.decode_case(fixture, "c2_")[0].shape) == (2, 67, 131)


@pytest.mark.parametrize("tree", ["jdacs", "jdacs-ms"])
def test_oracle_vs_live_reference(fixture, tree):
    """The restatement against the reference's functions imported from its tree: the same bits on the same CPU, every case."""
    if not os.path.isdir(os.path.join(REF, tree)):
        pytest.skip("the reference tree is not on this machine")
    fns = M.reference_functions(REF, tree)
    for prefix in M.CASES:
        est, gt, mask, interval = M.decode_case(fixture, prefix)
        r_out, r_per = M.reference_values(fns, est, gt, mask, interval)
        o32, p32 = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float32)
        assert M.same_bits(o32, r_out) and M.same_bits(p32, r_per), (tree, prefix)


@pytest.mark.parametrize("prefix", M.CASES)
def test_depth_metrics_emulated_vs_fixture(emul_lib, fixture, prefix):
    """ops.depth_metrics through the emulated kernels on every case, by the metrics' criteria; a bool mask, its fp32 form and its
    uint8 form give the same bits; a second run gives the same bits; the inputs are not modified."""
    est, gt, mask, interval = M.decode_case(fixture, prefix)
    r_out, r_per, t_out, t_per = M.fixture_results(fixture, prefix)
    e0, g0 = est.clone(), gt.clone()
    emul_lib.launch_trace()
    out, per = _ours(est, gt, mask, interval)
    assert emul_lib.launch_trace() == ["depth_metrics_partial", "depth_metrics_finish"]
    assert tuple(out.shape) == (4 + T,) and tuple(per.shape) == (est.shape[0], 2 + T)
    assert out.dtype == per.dtype == torch.float32 and not out.requires_grad
    assert M.same_bits(est, e0) and torch.equal(gt, g0)
    M.check_against(out, per, r_out, r_per, t_out, t_per, T, what=prefix + "emul")
    for other in (mask.float(), mask.to(torch.uint8), mask):
        o2, p2 = _ours(est, gt, other, interval)
        assert M.same_bits(o2, out) and M.same_bits(p2, per), other.dtype


@pytest.mark.parametrize("prefix", M.CASES)
def test_dropins_of_both_trees_vs_fixture(emul_lib, fixture, prefix):
    """Thres_metrics, AbsDepthError_metrics, the three interval metrics and depth_metrics() under the reference's names and call
    signatures, from mvs_amd.jdacs and mvs_amd.jdacs_ms: 0-dim tensors with the bits of the one-call form, by the criteria."""
    from mvs_amd.jdacs import utils as U
    from mvs_amd.jdacs.losses import unsup_loss as L
    from mvs_amd.jdacs_ms import utils as U2
    from mvs_amd.jdacs_ms.losses import unsup_loss as L2
    est, gt, mask, interval = M.decode_case(fixture, prefix)
    r_out, r_per, t_out, t_per = M.fixture_results(fixture, prefix)
    out, per = _ours(est, gt, mask, interval)
    fmask = mask.float()
    for u, l in ((U, L), (U2, L2)):
        vals = [u.AbsDepthError_metrics(est, gt, fmask > 0.5)] + [u.Thres_metrics(est, gt, fmask > 0.5, t) for t in M.THRESHOLDS] + \
               [l.non_zero_mean_absolute_diff(gt, est, interval), l.less_one_percentage(gt, est, interval),
                l.less_three_percentage(gt, est, interval)]
        assert all(v.dim() == 0 and v.dtype == torch.float32 and not v.requires_grad for v in vals)
        got = torch.stack(vals)
        assert M.same_bits(got, out), (got, out)
        M.check_against(got, per, r_out, r_per, t_out, t_per, T, what=prefix + u.__name__)
        d = u.depth_metrics(est, gt, fmask, interval)
        assert tuple(d) == M.KEYS == u.METRIC_KEYS and M.same_bits(torch.stack([d[k] for k in M.KEYS]), out)
    with pytest.raises(AssertionError):
        U.Thres_metrics(est, gt, mask, torch.tensor(2.0))          # the reference's assert on the threshold's type stays
    est_g = est.clone().requires_grad_(True)
    assert not U.AbsDepthError_metrics(est_g * 1.0, gt, mask).requires_grad


def test_tiles_alignment_and_non_contiguous_inputs(emul_lib, fixture):
    """Case 2 spreads over three tiles per image (workspace-size entry); the same pixels behind an odd offset (scalar loads), as
    non-contiguous views, and as a [B, HW] shape give the bits of the aligned, contiguous run; without an interval the three
    interval metrics are NaN and the other four unchanged; T = 0 and T = 8 work."""
    from mvs_amd import ops
    est, gt, mask, interval = M.decode_case(fixture, "c2_")
    b, h, w = est.shape
    assert h * w > 2 * 4096 and (h * w) % 4096 != 0
    assert emul_lib.raw("mvs_depth_metrics_workspace_bytes", b, h * w, T) == b * 3 * 64
    out, per = _ours(est, gt, mask, interval)

    def shifted(x, off):
        buf = torch.zeros(x.numel() + off, dtype=x.dtype)
        buf[off:] = x.reshape(-1)
        return buf[off:].view(x.shape)
    for off in (1, 2, 3):
        o2, p2 = _ours(shifted(est, off), shifted(gt, (off + 1) % 4), shifted(mask, off), interval)
        assert M.same_bits(o2, out) and M.same_bits(p2, per), off
        o2, p2 = _ours(shifted(est, off), shifted(gt, off), shifted(mask.float(), 3), interval)
        assert M.same_bits(o2, out) and M.same_bits(p2, per), off
    wide = lambda x: torch.stack([x, x.flip(0)], dim=-1)[..., 0]            # stride 2 along the row
    assert not wide(est).is_contiguous()
    o2, p2 = _ours(wide(est), wide(gt).transpose(1, 2).contiguous().transpose(1, 2), wide(mask), interval.view(b, 1, 1).expand(b, 1, 1))
    assert M.same_bits(o2, out) and M.same_bits(p2, per)
    o2, p2 = _ours(est.view(b, h * w), gt.view(b, h * w), mask.view(b, h * w), interval)
    assert M.same_bits(o2, out) and M.same_bits(p2, per)
    o3, p3 = _ours(est, gt, mask, None)
    assert torch.equal(o3[:1 + T], out[:1 + T]) and bool(torch.isnan(o3[1 + T:]).all())
    assert torch.equal(p3[:, :1 + T], per[:, :1 + T]) and bool(torch.isnan(p3[:, 1 + T]).all())
    o0, p0 = ops.depth_metrics(est, gt, mask, interval, ())
    assert torch.equal(o0, out[[0, 1 + T, 2 + T, 3 + T]]) and torch.equal(p0, per[:, [0, 1 + T]])
    eight = (0.5, 1, 2, 3, 4, 6, 8, 16)
    o8, p8 = ops.depth_metrics(est, gt, mask, interval, eight)
    r8, rp8 = M.seven(est, gt, mask, interval, eight, torch.float32)
    t8, tp8 = M.seven(est, gt, mask, interval, eight, torch.float64)
    M.check_against(o8, p8, r8, rp8, t8, tp8, 8, what="T=8")
    assert torch.equal(o8[[3, 5, 7]], out[1:1 + T])


def test_more_images_than_one_finish_pass(emul_lib):
    """B = 20 small images: the finish kernel serves 16 images per pass, so this takes two; one image's mask is empty."""
    from mvs_amd import ops
    est, gt, mask, interval = M.seeded_inputs(20, 5, 7, seed=181)
    mask[17] = 0
    r_out, r_per = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float32)
    t_out, t_per = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float64)
    out, per = ops.depth_metrics(est, gt, mask, interval, M.THRESHOLDS)
    assert bool(torch.isnan(per[17, :1 + T]).all()) and int(torch.isnan(per).sum()) == 1 + T and bool(torch.isnan(out[:1 + T]).all())
    M.check_against(out, per, r_out, r_per, t_out, t_per, T, what="B=20")
    for b in range(20):                                       # per image: the single-image call's bits
        o1, p1 = ops.depth_metrics(est[b:b + 1], gt[b:b + 1], mask[b:b + 1], interval[b:b + 1], M.THRESHOLDS)
        assert M.same_bits(p1[0], per[b]), b


def test_meter_mean_after_three_updates(emul_lib, fixture):
    """DepthMetricsMeter: mean() after three updates is the mean of the three out vectors (fp64 sums of the fp32 values, as
    DictAverageMeter forms them from tensor2float's Python floats), under DictAverageMeter.mean()'s keys."""
    from mvs_amd.jdacs.utils import DepthMetricsMeter, DictAverageMeter, tensor2float
    from mvs_amd.jdacs_ms.utils import DepthMetricsMeter as Meter2
    assert Meter2 is DepthMetricsMeter
    meter, ref_meter, outs = DepthMetricsMeter(), DictAverageMeter(), []
    assert meter.count == 0
    for prefix in ("c1_", "c2_", "c6_"):
        est, gt, mask, interval = M.decode_case(fixture, prefix)
        d = meter.update(est, gt, mask.float(), interval)
        outs.append(_ours(est, gt, mask, interval)[0])
        assert M.same_bits(torch.stack([d[k] for k in M.KEYS]), outs[-1])
        ref_meter.update(tensor2float(d))
    assert meter.count == 3
    mean, want = meter.mean(), ref_meter.mean()
    assert tuple(mean) == tuple(want) == M.KEYS
    expect = torch.stack(outs).double().sum(0) / 3
    for i, k in enumerate(M.KEYS):
        assert mean[k] == want[k] == float(expect[i]), k
    with pytest.raises(RuntimeError, match="before any update"):
        DepthMetricsMeter().mean()
    with pytest.raises(ValueError, match="meter must be"):
        est, gt, mask, interval = M.decode_case(fixture, "c6_")
        _ours(est, gt, mask, interval, meter=(torch.zeros(7), torch.zeros(1, dtype=torch.int64)))


def test_generic_helpers_keep_the_reference_behaviour():
    """make_nograd_func, compute_metrics_for_each_image (for a caller's own metric) and DictAverageMeter on plain CPU tensors."""
    from mvs_amd.jdacs.utils import DictAverageMeter, compute_metrics_for_each_image, make_nograd_func

    @make_nograd_func
    @compute_metrics_for_each_image
    def masked_max(e, g, m, scale):
        return (e[m] - g[m]).abs().max() * scale
    e = torch.arange(24.0).view(2, 3, 4).requires_grad_(True)
    g = torch.zeros(2, 3, 4)
    m = torch.ones(2, 3, 4, dtype=torch.bool)
    v = masked_max(e, g, m, 2.0)
    assert float(v) == (11 * 2 + 23 * 2) / 2 and not v.requires_grad
    meter = DictAverageMeter()
    meter.update({"a": 1.0, "b": 4.0})
    meter.update({"a": 2.0, "b": 0.0})
    assert meter.mean() == {"a": 1.5, "b": 2.0} and meter.count == 2
    with pytest.raises(NotImplementedError, match="invalid data"):
        meter.update({"a": torch.tensor(1.0)})


def test_error_paths(emul_lib, fixture):
    from mvs_amd import ops
    est, gt, mask, interval = M.decode_case(fixture, "c6_")
    with pytest.raises(ValueError, match="share one"):
        ops.depth_metrics(est, gt[:, :-1], mask, interval)
    with pytest.raises(ValueError, match="share one"):
        ops.depth_metrics(est, gt, mask[:1], interval)
    with pytest.raises(ValueError, match="0 <= T <= 8"):
        ops.depth_metrics(est, gt, mask, interval, tuple(range(9)))
    with pytest.raises(ValueError, match="interval must hold B = 2"):
        ops.depth_metrics(est, gt, mask, torch.ones(3))
    with pytest.raises(TypeError, match="mask must be"):
        ops.depth_metrics(est, gt, mask.double(), interval)
    with pytest.raises(TypeError, match="fp32 tensors required"):
        ops.depth_metrics(est.double(), gt, mask, interval)


def _product_lib():
    from mvs_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.MvsLib()


def test_cpu_tensors_are_rejected_by_the_product_library(fixture, monkeypatch):
    from mvs_amd import _lib, ops
    from mvs_amd.jdacs.utils import AbsDepthError_metrics
    _product_lib()
    monkeypatch.setattr(_lib, "_INSTANCE", None)         # the next ops call loads the product library
    est, gt, mask, interval = M.decode_case(fixture, "c6_")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_metrics(est, gt, mask, interval)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AbsDepthError_metrics(est, gt, mask)


def test_entry_point_rejects_bad_arguments():
    """mvs_depth_metrics: null pointers and every limit are rejected on the host before any launch, with a message; the workspace
    query answers -1 for the same sizes and B * ceil(HW / 4096) * 64 otherwise (product library, no GPU needed)."""
    lib = _product_lib()
    d = C.c_void_p(64)                      # never dereferenced
    th = (C.c_float * 8)(*range(8))

    def call(est=d, gt=d, mask=d, interval=d, thres=th, t=3, b=2, hw=100, ws=d, out=d, per=d, meter=None, count=None):
        lib.call("mvs_depth_metrics", est, gt, mask, 1, interval, thres, t, b, hw, ws, out, per, meter, count, None)
    lib.launch_trace()
    for kw in ({"est": None}, {"gt": None}, {"mask": None}, {"ws": None}, {"out": None}, {"per": None}, {"thres": None}):
        with pytest.raises(ValueError, match="null pointer"):
            call(**kw)
    for kw in ({"meter": d}, {"count": d}):
        with pytest.raises(ValueError, match="go together"):
            call(**kw)
    for kw, msg in (({"t": 9}, "0 <= T <= 8"), ({"t": -1}, "0 <= T <= 8"), ({"b": 0}, "1 <= B <= 65535"), ({"b": -3}, "1 <= B"),
                    ({"b": 65536}, "1 <= B <= 65535"), ({"hw": 0}, "HW >= 1"), ({"hw": -5}, "HW >= 1")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    for b, hw, t in ((0, 100, 3), (2, 0, 3), (2, 100, 9), (2, 100, -1), (65536, 100, 3)):
        assert lib.raw("mvs_depth_metrics_workspace_bytes", b, hw, t) == -1
    for b, hw, t in ((1, 1, 0), (4, 128 * 160, 3), (1, 1200 * 1600, 3), (2, 67 * 131, 8), (3, 4096, 1), (3, 4097, 1)):
        assert lib.raw("mvs_depth_metrics_workspace_bytes", b, hw, t) == b * ((hw + 4095) // 4096) * 64
    assert lib.raw("mvs_depth_metrics_workspace_bytes", 4, 128 * 160, 3) == 4 * 5 * 64       # several workgroups per training map
    assert lib.launch_trace() == []


def test_source_enqueues_only_and_has_no_atomics():
    """csrc/depth_metrics_kernels.h holds no stream / device / event synchronisation, no device-to-host copy, no atomics and no
    wave shuffles (the emulation has them for float and int only): two enqueued launches, sums through LDS in a fixed order."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "self-supervised-mvs_amd", "csrc", "depth_metrics_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("Synchronize", "hipMemcpy", "hipStreamQuery", "hipEventQuery", "hipHostMalloc", "hipStreamWaitEvent", "atomic",
                 "volatile", "__threadfence", "__shfl", "while ("):
        assert word not in code, word
    assert "mvs_depth_metrics" in code and code.count("MVS_LAUNCH(") == 3          # two byte / fp32 mask arms + the finish
    assert "depth_metrics_kernels.h" in open(os.path.join(root, "self-supervised-mvs_amd", "csrc", "loss.hip")).read()
    assert "depth_metrics_kernels.h" in open(os.path.join(root, "self-supervised-mvs_amd", "csrc", "Makefile")).read()
