"""GPU parity of the size-selected conv3d arms (-m gpu): run_igemm / run_cin1 / run_wgrad (csrc/conv3d.hip) pick a kernel by launch
size and by knobs, and test_conv3d_family_vs_torch's shapes all fall to the generic one-tile arms.  Every test here forces or
reaches ONE arm, proves through the launch trace (mvs_launch_trace) that this arm and not the generic one ran, and compares it with
F.conv3d / F.conv_transpose3d (+ the epilogue written out in torch) on the CPU in float64, ATen's float32 result being the yardstick
(conftest criteria, default slack 4).  The case table lives in tests/conv_arm_cases.py; tests/test_conv_arm_dispatch.py checks the
same traces on the emulation build without a GPU.

Which test is the GPU record for which arm:
  test_conv_pers_forward                 conv_pers_kernel forward, SIDE = 0 and SIDE = 1 (skip), scale/shift/ReLU/statistics, forced
                                         (conv_pers_min = 0; conv_pers_groups 3 and 0): S1 CC 16, S2 CC 8, TR2_PW, S1 CC 8 with two Cout tiles
  test_conv_pers_input_gradient          the same kernel as input gradient with summand + BatchNorm backward statistics, through
                                         mvs_conv3d_dgrad and mvs_convT3d_dgrad
  test_conv_pers_default_dispatch        the same kernel picked by the library itself (no knob), >= 3 ragged tiles per workgroup
  test_conv_pers_four_waves              conv_pers_kernel<.., NW = 4> (knob conv_pers_nw)
  test_conv_wgrad_pers                   conv_wgrad_pers_kernel<S1, 16> / <S2, 8>, forced and by default dispatch
  test_conv_wgrad_small_tiles            conv_wgrad_kernel<*_SMALL, CC, nbw 1 / 2> (knob wgrad_small = 3)
  test_conv_wgrad_reduce_wide_and_narrow conv_wgrad_reduce_wide_kernel / conv_wgrad_reduce_kernel on one layer
  test_conv_cout1_forms                  conv_cout1_h4_kernel, conv_cout1_kernel<8>, <16>
  test_conv_cin1_input_gradient          conv_cin1_kernel<C, 1> / <C, 4> with backward statistics
  test_conv_auto_tiling                  conv_igemm_kernel under conv_small = 1 (the default), either side of conv_small_wgs
  test_conv_c8_and_cg1_arms              conv_c8_fwd_bc_kernel, conv_c8_wgrad_gs_kernel, conv_c8_wgrad_kernel, conv_wgrad_cg1_mfma_kernel: label and
                                         kernel tied together (their shape coverage is test_gpu_parity.py's)
  test_conv3d_stride2_input_gradient_rejects_odd_dims   the host's limit on mvs_conv3d_dgrad at stride 2

Where the double buffer wraps (a workgroup walks >= 3 tiles): every groups_3 variant (16 tiles over 3 workgroups; 8 for
dgrad_16_16_s1 / dgrad_32_8_s1) and the default-dispatch cases (800-1540 tiles over 256 / 512 workgroups).

Per-case error ratios (ours / ATen fp32, both against fp64) are appended to the file MVS_ARM_REPORT names (or to
conv_arm_parity_ratios.jsonl next to MVS_GRAD_REPORT's file, when only that is set); the copy kept with the project is profiles/conv_arm_parity_ratios.jsonl."""
import json
import os

import pytest
import torch

import conv_arm_cases as K
from conftest import assert_as_accurate_as_fp32_reference, assert_grads_as_accurate_as_fp32_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from mvs_amd import _lib
    _lib._INSTANCE = None
    lib = _lib.get()
    assert lib.raw("mvs_is_emulation") == 0  # the product library, not the test emulation
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def knob_defaults(dev):
    """no test before this module left a knob changed (every case scopes its own: lib.tuning)"""
    from mvs_amd import _lib
    for k, v in _lib.DEFAULT_TUNING.items():
        assert _lib.get().get_tuning(k) == v, "a test before this module left knob %s changed" % k


def _report(row):
    out = os.environ.get("MVS_ARM_REPORT", "")
    if not out and os.environ.get("MVS_GRAD_REPORT"):       # next to the gradient-ratio report of conftest.record_grad_report
        out = os.path.join(os.path.dirname(os.path.abspath(os.environ["MVS_GRAD_REPORT"])), "conv_arm_parity_ratios.jsonl")
    if not out:
        return
    try:
        with open(out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
    except OSError:
        pass


def _ratios(ours, ref32, truth64):
    t = truth64.float()
    e_o, e_r = (ours - t).abs(), (ref32 - t).abs()
    return {"max_err": float(e_o.max()), "max_err_fp32": float(e_r.max()), "mean_err": float(e_o.mean()), "mean_err_fp32": float(e_r.mean()),
            "max_ratio": float(e_o.max()) / max(float(e_r.max()), 1e-300), "mean_ratio": float(e_o.mean()) / max(float(e_r.mean()), 1e-300)}


def _check_stats(case, name, got, truth):
    """BatchNorm statistic slots against fp64 sums of the fp64 truth (the family test's tolerances)"""
    if truth is None:
        assert got is None
        return
    got = got.cpu()
    for i in (0, 1):
        assert torch.allclose(got[i], truth[i], atol=5e-2, rtol=1e-4), \
            "%s/%s statistic %d: %s vs %s" % (case.id, name, i, got[i].tolist(), truth[i].tolist())


def _check_case(case, dev):
    from mvs_amd import _lib
    lib = _lib.get()
    inp = K.make_inputs(case)
    t64, r32 = K.reference(case, inp, torch.float64), K.reference(case, inp, torch.float32)
    dinp = K.to_device(inp, dev)
    pers = any("pers" in lab for v in case.variants for lab in v.trace)
    base = None
    if case.base is not None:
        with lib.tuning(**case.base.knobs):
            lib.launch_trace()
            base = K.run(case, dinp, lib)["out"].cpu()
            assert lib.launch_trace() == case.base.trace, case.id
    for v in case.variants:
        what = "%s/%s" % (case.id, v.name)
        with lib.tuning(**v.knobs):
            lib.launch_trace()
            first = K.run(case, dinp, lib)
            trace = lib.launch_trace()
            second = K.run(case, dinp, lib)
            # which arm ran
            assert trace == v.trace, "%s took %s" % (what, trace)
            if pers:
                assert not any(lab.startswith(g) for lab in trace for g in K.GENERIC_LABELS), "%s fell through to the generic arm: %s" % (what, trace)
            out = first["out"].cpu()
            # no float atomics in the output path: two calls agree bit for bit (a staging race shows here first)
            assert torch.equal(out, second["out"].cpu()), "%s: two calls differ by %.3e" % (what, float((out - second["out"].cpu()).abs().max()))
            ratios = _ratios(out, r32["out"], t64["out"])
            print("%s: %s" % (what, json.dumps(ratios)))
            _report(dict(ratios, case=case.id, variant=v.name, op=case.op, trace=trace, slack_allowed=4.0))
            if case.op == "wgrad":
                assert_grads_as_accurate_as_fp32_reference({"w": out}, {"w": r32["out"]}, {"w": t64["out"]}, what=what)
                bound = 1e-3 * max(1.0, float(t64["out"].abs().max()))
            else:
                assert_as_accurate_as_fp32_reference(out, r32["out"], t64["out"], what=what)
                bound = 3e-4 if case.op in ("fwd", "fwd1") else 5e-4
            assert ratios["max_err"] < bound, "%s: max err %.3e over the family test's bound %.1e" % (what, ratios["max_err"], bound)
            _check_stats(case, v.name, first["stats"], t64["stats"])
            _check_stats(case, v.name, second["stats"], t64["stats"])
            # against the arm it replaces, identical inputs
            if base is not None and case.bitwise:
                assert torch.equal(out, base), "%s differs from the one-tile kernel by %.3e" % (what, float((out - base).abs().max()))
            elif base is not None:
                scale = max(1.0, float(t64["out"].abs().max()))
                assert float((out - base).abs().max()) < 2e-4 * scale, what


@pytest.mark.parametrize("case", K.PERS_FWD, ids=K.ids(K.PERS_FWD))
def test_conv_pers_forward(dev, knob_defaults, case):
    """conv_pers_kernel forward (label conv_pers), forced with conv_pers_min = 0, three persistent workgroups and one tile per
    workgroup; raw output + statistics, and scale / shift / ReLU / skip (the SIDE = 1 instantiation) + statistics; bitwise equal
    to the one-tile kernel (conv_igemm) it replaces."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.PERS_DGRAD, ids=K.ids(K.PERS_DGRAD))
def test_conv_pers_input_gradient(dev, knob_defaults, case):
    """conv_pers_kernel as input gradient with summand and BatchNorm backward statistics (add=, bn=), through mvs_conv3d_dgrad
    (stride 1: flipped taps; stride 2: TR2_PW) and mvs_convT3d_dgrad (stride-2 geometry)."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.PERS_DEFAULT, ids=K.ids(K.PERS_DEFAULT))
def test_conv_pers_default_dispatch(dev, knob_defaults, case):
    """No knob set: shapes ragged in D, H and W, large enough that the library itself takes conv_pers with at least three tiles
    for each of its 256 / 512 workgroups."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.PERS_NW4, ids=K.ids(K.PERS_NW4))
def test_conv_pers_four_waves(dev, knob_defaults, case):
    """The four-wave instantiations of conv_pers_kernel (knob conv_pers_nw = 4; label conv_pers nw=4)."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.WGRAD_PERS, ids=K.ids(K.WGRAD_PERS))
def test_conv_wgrad_pers(dev, knob_defaults, case):
    """conv_wgrad_pers_kernel (label conv_wgrad_pers) against fp64 autograd and against the register-staged conv_wgrad kernel it
    replaces (another split of the K sum: 2e-4 x scale, not bitwise)."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.WGRAD_SMALL, ids=K.ids(K.WGRAD_SMALL))
def test_conv_wgrad_small_tiles(dev, knob_defaults, case):
    """conv_wgrad_kernel on the *_SMALL geometries (label conv_wgrad (small tiles)), one and two gradient-channel tiles."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.WGRAD_REDUCE, ids=K.ids(K.WGRAD_REDUCE))
def test_conv_wgrad_reduce_wide_and_narrow(dev, knob_defaults, case):
    """conv_wgrad_reduce_wide_kernel (> 32 partial images) and conv_wgrad_reduce_kernel (label conv_wgrad_reduce wide / narrow)
    behind the same conv_wgrad launch."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.COUT1, ids=K.ids(K.COUT1))
def test_conv_cout1_forms(dev, knob_defaults, case):
    """The Cout == 1 forward kernels with their bias (label conv_cout1 h4 / cin=8 / cin=16); ragged 4 x 8 x 32 and 4 x 4 x 16 tiles."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.CIN1, ids=K.ids(K.CIN1))
def test_conv_cin1_input_gradient(dev, knob_defaults, case):
    """conv_cin1_kernel<C, 1> and <C, 4> (label conv_cin1 vpt=1 / vpt=4) with BatchNorm backward statistics; the last workgroup
    of either form is partly past the volume."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.AUTO, ids=K.ids(K.AUTO))
def test_conv_auto_tiling(dev, knob_defaults, case):
    """conv_small = 1 (the library default): the trace says which tiling the generic kernel took (label conv_igemm s1 / s1_small /
    s2 / s2_small)."""
    _check_case(case, dev)


@pytest.mark.parametrize("case", K.C8_CG1, ids=K.ids(K.C8_CG1))
def test_conv_c8_and_cg1_arms(dev, knob_defaults, case):
    """The Cout == 8 broadcast-operand forward (label conv_c8_fwd_bc), conv0's two weight-gradient forms (conv_c8_wgrad_gs,
    conv_c8_wgrad) and the Cout == 1 weight gradient (conv_wgrad_cg1): the trace ties each label to its kernel."""
    _check_case(case, dev)


# every launch label of csrc/conv3d.hip and csrc/conv3d_pers.hip
ARM_LABELS = ("conv_pers nw=8", "conv_pers nw=4", "conv_wgrad_pers", "conv_igemm s1", "conv_igemm s2", "conv_igemm s1_small",
              "conv_igemm s2_small", "conv_igemm tr2_pw", "conv_cout1 h4", "conv_cout1 cin=8", "conv_cout1 cin=16", "conv_cin1 vpt=1",
              "conv_cin1 vpt=4", "conv_wgrad nbw=1", "conv_wgrad nbw=2", "conv_wgrad (small tiles) nbw=1", "conv_wgrad (small tiles) nbw=2",
              "conv_wgrad_cg1", "conv_c8_fwd_bc", "conv_c8_wgrad", "conv_c8_wgrad_gs", "conv_wgrad_reduce wide", "conv_wgrad_reduce narrow",
              "conv_pack_weights")


def test_every_arm_label_is_asserted_by_a_case():
    """each label above is in the exact trace some case of this file asserts"""
    groups = (K.PERS_FWD, K.PERS_DGRAD, K.PERS_DEFAULT, K.PERS_NW4, K.WGRAD_PERS, K.WGRAD_SMALL, K.WGRAD_REDUCE, K.COUT1, K.CIN1, K.AUTO,
              K.C8_CG1)
    seen = {lab for grp in groups for c in grp for v in list(c.variants) + ([c.base] if c.base else []) for lab in v.trace}
    assert set(ARM_LABELS) <= seen, set(ARM_LABELS) - seen


@pytest.mark.parametrize("dims", [(5, 8, 10), (6, 7, 10), (6, 8, 9)], ids=["odd_depth", "odd_height", "odd_width"])
def test_conv3d_stride2_input_gradient_rejects_odd_dims(dev, dims):
    """The input gradient of a stride-2 convolution runs as a transposed convolution over the output gradient's grid and writes
    2 x that grid: an odd input dimension is not served, and the host says so before anything is launched (which is why
    test_conv3d_family_vs_torch leaves that gradient out for its 5 x 7 x 9 case)."""
    from mvs_amd import ops
    gy = torch.zeros(2, 32, *[(s - 1) // 2 + 1 for s in dims], device=dev)
    w = torch.zeros(32, 16, 3, 3, 3, device=dev)
    with pytest.raises(ValueError, match=r"conv3d_dgrad stride 2: D,H,W must be even, got %d x %d x %d" % dims):
        ops.conv3d_dgrad(gy, w, (2, 16) + dims, 2, False)
