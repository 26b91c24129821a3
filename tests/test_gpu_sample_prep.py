"""GPU (MI355X): training-sample preparation (csrc/sample_prep_kernels.h: mvs_sample_prep) on the device -- the shapes and criteria
of tests/test_sample_prep.py's emulation test with the fp32 restatement evaluated on the same GPU, determinism, NCHW against
channels-last, the launch trace, no host synchronisation, and SamplePrep's tensors fed to MVSNet."""
import numpy as np
import pytest
import torch

import sample_prep_oracle as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from mvs_amd import _lib
    _lib._INSTANCE = None
    lib = _lib.get()
    assert lib.raw("mvs_is_emulation") == 0  # the product library, not the test emulation
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(P.CASES))
def test_cases_vs_oracle_on_the_device(dev, name):
    """(1, 5, 7) smaller than a tile; (3, 37, 53) odd pixel count, unaligned image offsets, H / 4 and W / 4 floored; (5, 128, 160)
    several tiles; (2, 130, 1030) a ragged last tile; (2, 40, 48) read as a 32-row crop through the image stride; 24 views, one
    per operation order.  Criteria of the issue against the fp32 and fp64 restatement on this GPU; exactly three launches inside
    one C call; a second run gives the same bits; the channels-last outputs are equal element by element."""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    stored, _, table, rects = P.make_case(name)
    M, H, W, rows, N = P.CASES[name]
    used = stored.to(dev)[:, :rows]
    assert used.is_contiguous() == (rows == H)
    o32 = P.prepare(used.contiguous(), table, rects, torch.float32, mask_scale=4)
    o64 = P.prepare(used.contiguous(), table, rects, torch.float64, mask_scale=4)
    timer = _lib.KernelTimer(names={"mvs_sample_prep"})
    lib.launch_trace()
    lib.profiler = timer
    try:
        out = ops.sample_prep(used, table, rects, mask_scale=4)
    finally:
        lib.profiler = None
    assert lib.launch_trace() == ["sample_prep_stats", "sample_prep_aug_stats", "sample_prep_write"]
    torch.cuda.synchronize()
    assert [(k[0], v[0]) for k, v in timer.summary().items()] == [("mvs_sample_prep", 1)]
    assert all(v.device.type == "cuda" for v in out.values())
    P.check_outputs(out, o32, o64, what=name + " gpu")
    again = ops.sample_prep(used, table, rects, mask_scale=4)
    cl = ops.sample_prep(used, table, rects, mask_scale=4, channels_last=True)
    for k, v in out.items():
        assert torch.equal(again[k], v), k
        assert torch.equal(cl[k], v), k
        if k != "filter_mask":
            assert cl[k].permute(0, 2, 3, 1).is_contiguous() and v.is_contiguous()
    lib.launch_trace()
    plain = ops.sample_prep(used, None, None)
    assert lib.launch_trace() == ["sample_prep_stats", "sample_prep_write"]              # two without a table
    assert sorted(plain) == ["imgs", "imgs_seg"] and torch.equal(plain["imgs"], out["imgs"])


def test_more_views_than_one_group_of_launches(dev):
    """70 views of 6 x 10: two groups of 64 views' parameters, six launches, every view with its own table row and window"""
    from mvs_amd import _lib, ops
    lib = _lib.get()
    views = P.seeded_views(70, 6, 10, 631).to(dev)
    table = P.seeded_table(70, 632, first_order=3, gammas=())
    low = (table[:, :4] <= 1) & (table[:, 4:8] < 0.5)         # brightness / contrast factors near 0 leave a nearly constant view,
    table[:, 4:8][low] = 0.5                                  # whose centring divides by ~0: ill-conditioned for every evaluation
    rects = np.zeros((70, 4), np.int32)
    rects[::7] = (1, 2, 1, 2)
    o32 = P.prepare(views, table, rects, torch.float32, mask_scale=1)
    o64 = P.prepare(views, table, rects, torch.float64, mask_scale=1)
    lib.launch_trace()
    out = ops.sample_prep(views, table, rects, mask_scale=1)
    assert lib.launch_trace() == ["sample_prep_stats", "sample_prep_aug_stats", "sample_prep_write"] * 2
    P.check_outputs(out, o32, o64, what="70 views gpu")


def test_augmentor_form_on_the_device(dev):
    """src_kind 1 at (2 * 3, 36, 52): fp32 planes in [0, 1] quantised on load, brightness and contrast only, not centred, an
    (h // 4, w // 4) window on each sample's first view and the full-size mask; and the Augmentor module itself."""
    from mvs_amd import _lib, ops
    from mvs_amd.jdacs.models.augmentations import Augmentor
    from mvs_amd.sample_prep import SamplePrep
    lib = _lib.get()
    x, table, rects = P.augmentor_case()
    xd = x.to(dev)
    u8 = P.quantise(xd)
    assert torch.equal(u8.cpu(), P.quantise(x))
    o32 = P.prepare(u8, table, rects, torch.float32, aug_center=False, mask_scale=1)
    o64 = P.prepare(u8, table, rects, torch.float64, aug_center=False, mask_scale=1)
    lib.launch_trace()
    out = ops.sample_prep(xd, table, rects, imgs=False, seg=False, mask_scale=1, aug_center=False)
    assert lib.launch_trace() == ["sample_prep_stats", "sample_prep_write"]
    P.check_outputs(out, o32, {k: o64[k] for k in ("imgs_aug", "filter_mask")}, what="augmentor gpu")
    aug = Augmentor()
    np.random.seed(31)
    got, mask = aug(xd.view(2, 3, 3, 36, 52))
    np.random.seed(31)
    t2 = aug.transform.draw(2, 3)
    r2 = np.zeros((2, 3, 4), np.int32)
    r2[:, 0] = SamplePrep.window(2, 36, 52, (9, 13), np.random.mtrand._rand)
    want = ops.sample_prep(xd, t2, r2.reshape(6, 4), imgs=False, seg=False, mask_scale=1, aug_center=False)
    assert torch.equal(got.reshape(6, 3, 36, 52), want["imgs_aug"]) and tuple(mask.shape) == (2, 3, 36, 52)
    assert torch.equal(mask[:, 1], want["filter_mask"].view(2, 3, 36, 52)[:, 0])
    assert (t2[:3, :8] == t2[0, :8]).all() and len(set(t2[:3, 8].tolist())) == 3


def test_no_host_sync(dev):
    """ops.sample_prep, SamplePrep and Augmentor under torch.cuda.set_sync_debug_mode("error"): any host synchronisation raises."""
    from mvs_amd import ops
    from mvs_amd.jdacs.models.augmentations import Augmentor
    from mvs_amd.sample_prep import SamplePrep
    stored, _, table, rects = P.make_case("tiles")
    views = stored.to(dev)
    x01 = P.augmentor_case()[0].to(dev).view(2, 3, 3, 36, 52)
    prep, aug, rs = SamplePrep(), Augmentor(), np.random.RandomState(5)
    ops.sample_prep(views, table, rects, mask_scale=4)          # first use: library load, allocator warm-up
    aug(x01)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = ops.sample_prep(views, table, rects, mask_scale=4)
        b = prep(views.view(1, 5, 128, 160, 3), prep.draw(5, rs), prep.window(1, 128, 160, (42, 53), rs))
        c, m = aug(x01)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(b["imgs_aug"].shape) == (1, 5, 3, 128, 160) and tuple(b["filter_mask"].shape) == (1, 32, 40)
    assert torch.equal(b["imgs"].view(5, 3, 128, 160), a["imgs"]) and tuple(c.shape) == (2, 3, 3, 36, 52)


def test_sample_prep_feeds_mvsnet(dev):
    """SamplePrep's imgs and imgs_aug at (1, 3, 64, 96), D = 16, through MVSNet(refine=False).train(): forward and backward run
    and give finite values -- the tensors are what the model takes."""
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    from mvs_amd.sample_prep import SamplePrep
    from oracle import ref_torch as R
    torch.manual_seed(0)
    _, proj, dv = R.synthetic_mvsnet_inputs(1, 3, 64, 96, 16, seed=1)
    views = P.seeded_views(3, 64, 96, 641).view(1, 3, 64, 96, 3).to(dev)
    prep, rs = SamplePrep(), np.random.RandomState(9)
    s = prep(views, prep.draw(3, rs), prep.window(1, 64, 96, (21, 32), rs))
    assert tuple(s["imgs"].shape) == tuple(s["imgs_aug"].shape) == tuple(s["imgs_seg"].shape) == (1, 3, 3, 64, 96)
    assert tuple(s["filter_mask"].shape) == (1, 16, 24)
    net = MVSNet(refine=False).to(dev).train()
    for key in ("imgs", "imgs_aug"):
        net.zero_grad()
        depth = net(s[key], proj.to(dev), dv.to(dev))["depth"]
        assert tuple(depth.shape) == (1, 16, 24) and bool(torch.isfinite(depth).all())
        (depth * s["filter_mask"]).mean().backward()
        grads = [p.grad for p in net.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0
