"""GPU parity of the conv2d arms (-m gpu): csrc/conv2d.hip's host side picks between several dozen template instantiations by channel
counts, Cout tiles, the pixel-pair form, the BatchNorm epilogues and by knobs, and the other GPU tests' shapes (images >= 32 x 40,
whole-model rel_l1) cannot tell the arms apart.  Every case here runs ONE arm at the smallest shapes at which it can still go wrong
(1x1 ... 9x33; stride 2 up to 17x65: a tile is 8 x 32), proves through the launch trace (mvs_launch_trace) which instantiation ran, and
compares it with F.conv2d / autograd (+ the epilogue written out in torch) on the CPU in float64, ATen's float32 CPU result being the
yardstick (conftest criteria, default slack 4, + test_conv2d_family_vs_torch's absolute bounds).  Per case and variant: two calls --
one through mvs_amd.ops, one through lib.call on NaN-filled buffers of exactly the queried size with 1024 canary elements behind each
-- agree bit for bit; statistic slots (fp64 atomics) are compared with fp64 sums of the device's own output (STATS / XF) or with the
fp64 reference's sums (BST: yardstick = the fp32 CPU reference's sums); knob pairs on identical inputs to 2e-4 x scale, call forms
with the same arithmetic order bit for bit.  The case table lives in tests/conv2d_arm_cases.py; tests/test_conv2d_arm_dispatch.py checks
the same traces -- and the numbers of the cases of at most four tiles -- on the emulation build without a GPU.

Which test is the GPU record for which arm:
  test_conv2d_forward_arms             conv2d_igemm_kernel<3, 1, CC 4 / 8 / 16 / 32, NB 1 / 2> and <5, 2, 8, NB 1 / 2>, plain epilogue: grid.y = 2,
                                       two 32-channel chunks, scalar halo loads and stores, a partly filled second Cout tile; bias and
                                       LeakyReLU (mvs_conv2d_lrelu_fwd); channels-last parameters (mvs_conv2d_fwd_wl)
  test_conv2d_pixel_pairs              conv2d_igemm_kernel<3, 1, 4 / 8, 1, PP> against the plain kernel (knob conv2d_pp), forward and input
                                       gradient, the pair across the right edge (W = 1 / 31 / 33)
  test_conv2d_input_gradient_stride1   the same kernels on gy with the transposed, flipped image (mvs_conv2d_dgrad_wl)
  test_conv2d_forward_statistics       <.., STATS> (mvs_conv2d_fwd_stats, packed_ws or not): groups 1 / N / 2 of 4, slot wrap, y == plain y
  test_conv2d_forward_normalised_input <.., STATS, XF> (mvs_conv2d_fwd_stats_xf): negative scales, positive shifts, zero padding stays zero
  test_conv2d_input_gradient_bnstats   <.., STATS, false, BST> (mvs_conv2d_dgrad_bnstats), vector and scalar bn_raw loads
  test_conv2d_input_gradient_stride2   <3, 1, CC, NB, .., S2D> (one pass), the four-class form and conv2d_dgrad_s2_kernel (knob conv2d_s2_mfma)
  test_conv2d_weight_gradient          conv2d_wgrad_kernel<3 | 5, .., CXP, MT, NB>: all twelve, 64-channel slices, knob wgrad2d_groups 1 / 3
  test_conv2d_weight_gradient_reduce   conv2d_wgrad_reduce_kernel / conv2d_wgrad_reduce_wide_kernel either side of 16 partial images; 48 / 49 / 65
  test_conv2d_weight_gradient_batch    conv2d_wgrad_batch_kernel<0 / 1>, _xf0 / _xf1, conv2d_wgrad_batch_reduce_kernel: each config alone,
                                       FeatureNet's eight layers under wgrad2d_batch 1 / 6 / 20 / default, channels-last gradients
  test_conv2d_wgrad_refuses_what_it_has_no_instantiation_for   the served set of mvs_conv2d_wgrad on the product library

Per-case error figures (ours / ATen fp32, both against fp64) are appended to conv2d_arm_parity_ratios.jsonl in the folder of the file
MVS_ARM_REPORT (or MVS_GRAD_REPORT) names; the copy kept with the project is profiles/conv2d_arm_parity_ratios.jsonl."""
import pytest
import torch

import conv2d_arm_cases as K

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
    for k, v in (("conv2d_pp", 1), ("conv2d_s2_mfma", 2), ("wgrad2d_groups", 256)):
        assert _lib.get().get_tuning(k) == v, "a test before this module left knob %s changed" % k


def _two_calls(case, inp, lib, v):
    """on buffers the test owns (NaN-filled, canaries), then through the product's wrappers"""
    return [K.run_owned(case, inp, lib, v), K.run(case, inp, lib, v)]


def _check(case, dev):
    from mvs_amd import _lib
    K.check_numbers(case, _lib.get(), dev, _two_calls, record=K.report)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", K.FWD, ids=K.ids(K.FWD))
def test_conv2d_forward_arms(dev, knob_defaults, case):
    """Plain forward: every CC x NB of the 3x3 kernel and both NB of the 5x5 stride-2 kernel, with bias / LeakyReLU 0.1 at Cout 1 / 16 / 64,
    parameters contiguous and channels-last in memory (bit-identical: the packed image is the same)."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.PIXEL_PAIRS, ids=K.ids(K.PIXEL_PAIRS))
def test_conv2d_pixel_pairs(dev, knob_defaults, case):
    """conv2d_pp = 1 against 0 on identical inputs: the 12-tap pixel-pair image (the larger of the two workspace sizes) and the pair
    that straddles the right edge."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.DGRAD, ids=K.ids(K.DGRAD))
def test_conv2d_input_gradient_stride1(dev, knob_defaults, case):
    """The stride-1 input gradient: the forward kernels on gy with the transposed, flipped weight image; gx pre-filled with NaN."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.STATS, ids=K.ids(K.STATS))
def test_conv2d_forward_statistics(dev, knob_defaults, case):
    """The STATS epilogue: y bit-identical to the plain kernel's, the slot rows sum to fp64 sums of y and y^2 per statistics group, with
    fewer slot rows than workgroups (the caller-owned call) and more (the wrapper's mvs_bn_slots rows)."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.XF, ids=K.ids(K.XF))
def test_conv2d_forward_normalised_input(dev, knob_defaults, case):
    """The XF staging: relu(x * scale + shift) of the image's statistics group applied inside the image only."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.BST, ids=K.ids(K.BST))
def test_conv2d_input_gradient_bnstats(dev, knob_defaults, case):
    """The BST epilogue: gx as the plain input gradient, the slots = the BatchNorm block's backward sums, compared
    with the fp64 reference's; allowed: 4 x the error of the fp32 CPU reference's sums on the same inputs (+ conftest's 2e-6 floor).
    Both figures go to the report (bst_sums_err / bst_sums_err_fp32)."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.DGRAD_S2, ids=K.ids(K.DGRAD_S2))
def test_conv2d_input_gradient_stride2(dev, knob_defaults, case):
    """All three forms of the 5x5 stride-2 input gradient; gx pre-filled with NaN: every pixel belongs to exactly one parity class, an
    odd class may have no row / column at all, and the one-pass kernel's early return must not skip a live tile."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.WGRAD, ids=K.ids(K.WGRAD))
def test_conv2d_weight_gradient(dev, knob_defaults, case):
    """conv2d_wgrad_kernel, every instantiation; the workspace holds exactly the partial images of the knob's workgroup count."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.WGRAD_REDUCE, ids=K.ids(K.WGRAD_REDUCE))
def test_conv2d_weight_gradient_reduce(dev, knob_defaults, case):
    """The narrow reduce at 16 partial images, the wide one at 17 / 18 and at 48 / 49 / 65 (its unrolled loop's boundaries)."""
    _check(case, dev)


@pytest.mark.parametrize("case", K.WGRAD_BATCH, ids=K.ids(K.WGRAD_BATCH))
def test_conv2d_weight_gradient_batch(dev, knob_defaults, case):
    """mvs_conv2d_wgrad_batch(_xf): the workspace of mvs_conv2d_wgrad_batch_workspace_floats under each knob value, gradients in the
    parameters' own strides."""
    _check(case, dev)


def test_every_arm_label_is_asserted_by_a_case():
    """each launch label of the conv2d arms is in the exact trace some test of this file asserts"""
    groups = (K.FWD, K.PIXEL_PAIRS, K.DGRAD, K.STATS, K.XF, K.BST, K.DGRAD_S2, K.WGRAD, K.WGRAD_REDUCE, K.WGRAD_BATCH)
    seen = {lab for grp in groups for c in grp for v in c.variants for lab in v.trace}
    assert set(K.ARM_LABELS) <= seen, set(K.ARM_LABELS) - seen


@pytest.mark.parametrize("ks,cin", K.WGRAD_GAP)
def test_conv2d_wgrad_refuses_what_it_has_no_instantiation_for(dev, ks, cin):
    """mvs_conv2d_wgrad's served set on the product library: query -1, the wrapper's ValueError, nothing launched."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    stride = 2 if ks == 5 else 1
    ho, wo = K.out_hw((4, 6), stride)
    lib.launch_trace()
    assert lib.raw("mvs_conv2d_workspace_floats", 2, 1, 4, 6, cin, 64, ks, stride) == -1
    x = torch.zeros(1, cin, 4, 6, device=dev).contiguous(memory_format=K.CL)
    gy = torch.zeros(1, 64, ho, wo, device=dev).contiguous(memory_format=K.CL)
    with pytest.raises(ValueError, match="conv2d: unsupported shape .*weight gradient"):
        ops.conv2d_wgrad(x, gy, (64, cin, ks, ks), stride)
    assert lib.launch_trace() == []
