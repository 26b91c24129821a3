"""GPU (MI355X): the seven depth-map validation metrics (csrc/depth_metrics_kernels.h: mvs_depth_metrics) on the device -- the
reference's fixture cases, the test oracle at the training shape (B = 4, 128 x 160) and the dense-evaluation shape (B = 1,
1200 x 1600), determinism, two launches per call, and that neither ops.depth_metrics nor DepthMetricsMeter.update synchronises."""
import pytest
import torch

from conftest import load_golden
import metrics_oracle as M

pytestmark = pytest.mark.gpu
T = len(M.THRESHOLDS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from mvs_amd import _lib
    _lib._INSTANCE = None
    lib = _lib.get()
    assert lib.raw("mvs_is_emulation") == 0  # the product library, not the test emulation
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    return load_golden("g16_depth_metrics")


@pytest.mark.parametrize("prefix", M.CASES)
def test_fixture_cases_on_the_device(dev, fixture, prefix):
    """tests/test_depth_metrics.py::test_depth_metrics_emulated_vs_fixture on the device; case 2 runs three tiles per image."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    est, gt, mask, interval = M.decode_case(fixture, prefix)
    r_out, r_per, t_out, t_per = M.fixture_results(fixture, prefix)
    if prefix == "c2_":
        assert lib.raw("mvs_depth_metrics_workspace_bytes", est.shape[0], est.shape[1] * est.shape[2], T) == est.shape[0] * 3 * 64
    args = est.to(dev), gt.to(dev), mask.to(dev), interval.to(dev)
    lib.launch_trace()
    out, per = ops.depth_metrics(*args, M.THRESHOLDS)
    assert lib.launch_trace() == ["depth_metrics_partial", "depth_metrics_finish"]        # exactly two launches per call
    assert out.device.type == "cuda" and tuple(out.shape) == (4 + T,) and tuple(per.shape) == (est.shape[0], 2 + T)
    M.check_against(out.cpu(), per.cpu(), r_out, r_per, t_out, t_per, T, what=prefix + "gpu")
    o2, p2 = ops.depth_metrics(args[0], args[1], args[2].float(), args[3], M.THRESHOLDS)                 # fp32 mask: the same bits
    assert M.same_bits(o2.cpu(), out.cpu()) and M.same_bits(p2.cpu(), per.cpu())


@pytest.fixture(scope="module")
def big_cases(dev):
    """seeded inputs at the two shapes users run, with the oracle's fp32 and fp64 values computed once -- on the CPU, where the
    fixture generator asserts that the oracle reproduces the reference bit for bit (a device mean may multiply by 1 / n)"""
    cases = {}
    for name, (b, h, w, seed) in {"train": (4, 128, 160, 171), "dense": (1, 1200, 1600, 172)}.items():
        est, gt, mask, interval = M.seeded_inputs(b, h, w, seed)
        r = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float32)
        t = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float64)
        cases[name] = (est.to(dev), gt.to(dev), mask.to(dev), interval.to(dev), r, t)
    return cases


@pytest.mark.parametrize("name", ["train", "dense"])
def test_oracle_vs_device(dev, big_cases, name):
    """B = 4 at 128 x 160 (5 tiles per image) and B = 1 at 1200 x 1600 (469 tiles = 30 segments of the finish; 1.92 M pixels, below
    the 2^24 up to which the reference's fp32 counts are exact): by the metrics' criteria against the oracle's fp32 and fp64 values,
    with the fp32 mask train.py holds and with its bool form; a second run gives identical bits."""
    from mvs_amd import _lib, ops
    est, gt, mask, interval, (r_out, r_per), (t_out, t_per) = big_cases[name]
    b, hw = est.shape[0], est.shape[1] * est.shape[2]
    assert _lib.get().raw("mvs_depth_metrics_workspace_bytes", b, hw, T) == b * {"train": 5, "dense": 469}[name] * 64
    out, per = ops.depth_metrics(est, gt, mask, interval, M.THRESHOLDS)
    M.check_against(out.cpu(), per.cpu(), r_out, r_per, t_out, t_per, T, what=name)
    assert float(out[0]) > 0.5 and 0.0 < float(out[1]) < 1.0 and 0.0 < float(out[5]) < 1.0      # a non-degenerate case
    for m in (mask, mask > 0.5):
        o2, p2 = ops.depth_metrics(est, gt, m, interval, M.THRESHOLDS)
        assert torch.equal(o2, out) and torch.equal(p2, per)


def test_more_images_than_one_finish_pass(dev):
    """B = 20 images of 37 x 53 (the finish kernel serves 16 images per pass) against the oracle on the CPU."""
    from mvs_amd import ops
    est, gt, mask, interval = M.seeded_inputs(20, 37, 53, seed=182)
    r_out, r_per = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float32)
    t_out, t_per = M.seven(est, gt, mask, interval, M.THRESHOLDS, torch.float64)
    out, per = ops.depth_metrics(est.to(dev), gt.to(dev), mask.to(dev), interval.to(dev), M.THRESHOLDS)
    # the means over 20 images: 19 roundings of 2^-24 in another order stay below the 1e-6 the criterion allows for B <= 8 too
    M.check_against(out.cpu(), per.cpu(), r_out, r_per, t_out, t_per, T, what="B=20")


def test_no_host_sync_and_meter(dev, big_cases):
    """ops.depth_metrics, the drop-in dict and DepthMetricsMeter.update under torch.cuda.set_sync_debug_mode("error") (any host
    synchronisation raises); the meter's mean after three updates is the mean of the three out vectors."""
    from mvs_amd import ops
    from mvs_amd.jdacs.utils import DepthMetricsMeter, depth_metrics
    est, gt, mask, interval = big_cases["train"][:4]
    est2 = est + 0.25
    meter = DepthMetricsMeter()
    ops.depth_metrics(est, gt, mask, interval)          # first use: library load, allocator warm-up
    meter.update(est, gt, mask, interval)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out_a = ops.depth_metrics(est, gt, mask, interval)[0]
        out_b = ops.depth_metrics(est2, gt, mask > 0.5, interval)[0]
        d = depth_metrics(est, gt, mask, interval)
        meter.update(est2, gt, mask, interval)
        meter.update(est2, gt, mask, interval)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(torch.stack([d[k] for k in M.KEYS]), out_a)
    assert meter.count == 3
    mean = meter.mean()
    expect = (out_a.double() + 2 * out_b.double()).cpu() / 3
    for i, k in enumerate(M.KEYS):
        assert abs(mean[k] - float(expect[i])) <= 1e-12 * abs(float(expect[i])), k
