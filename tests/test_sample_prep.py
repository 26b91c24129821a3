"""CPU: training-sample preparation (csrc/sample_prep_kernels.h) -- the test-side restatement (tests/sample_prep_oracle.py) against
the reference's fixture (tests/golden/g17_sample_prep.npz), against PIL's ImageEnhance (the reference's real jitter path) and
against colorsys; ops.sample_prep, SamplePrep and Augmentor through the emulated kernels against the restatement; the parameter
draws; the entry point's argument checks against the product library."""
import colorsys
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import assert_as_accurate_as_fp32_reference, load_golden
from emul_util import emul_lib  # noqa: F401
import sample_prep_oracle as P

torch.set_num_threads(4)


@pytest.fixture(scope="module")
def fixture():
    return load_golden("g17_sample_prep")


# ---- the restatement against the reference's run ------------------------------------------------------------------------------------

def test_oracle_center_image_vs_fixture(fixture):
    """center_image of both trees on three 24 x 40 views and a constant one: the fp64 restatement within 1e-12 relative of the
    reference's statements run in fp64, the fp32 one as accurate as the reference's fp32 run; the constant image is exactly 0;
    jdacs-ms keeps the first 1184 of 1200 rows."""
    views = fixture["views"]
    assert tuple(views.shape) == (4, 24, 40, 3) and views.dtype == torch.uint8
    for m in range(4):
        o64, o32 = P.center_image(views[m].double()), P.center_image(views[m].float())
        t64, r32 = fixture["center64"][m], fixture["center32"][m]
        assert bool(((o64 - t64).abs() <= 1e-12 * t64.abs()).all()), m
        assert_as_accurate_as_fp32_reference(o32, r32, t64, what="center_image %d" % m)
    assert bool((fixture["center32"][3] == 0).all()) and bool((P.center_image(views[3].double()) == 0).all())
    assert bool((P.center_image(views[3].float()) == 0).all())
    tall = fixture["tall"]
    assert tuple(tall.shape) == (1200, 1, 3) and tuple(fixture["tall_center32"].shape) == (1184, 1, 3)
    assert_as_accurate_as_fp32_reference(P.center_image(tall[:1184].float()), fixture["tall_center32"],
                                         P.center_image(tall[:1184].double()), what="center_image 1200 -> 1184 rows")


def test_oracle_gamma_and_window_vs_fixture(fixture):
    """RandomGamma.adjust_gamma(clip_image=True) at gamma 0.5, 1, 2 (0^gamma = 0) and random_image_mask under its recorded seed:
    SamplePrep.window draws the same corner from a RandomState of that seed, x first."""
    from mvs_amd.sample_prep import SamplePrep
    u8 = fixture["views"][0, :6]
    assert int((u8 == 0).sum()) > 0
    for i, gamma in enumerate(fixture["gammas"].tolist()):
        row = [-1, -1, -1, -1, 1, 1, 1, 1, gamma]
        o64, o32 = P.chain(u8, row, torch.float64), P.chain(u8, row, torch.float32)
        t64 = fixture["gamma64"][i]
        assert bool(((o64 - t64).abs() <= 1e-12 * t64.abs()).all()), gamma
        assert_as_accurate_as_fp32_reference(o32, fixture["gamma32"][i], t64, what="gamma %g" % gamma)
        assert bool((o64[u8 == 0] == 0).all())
    fh, fw = fixture["mask_filter_size"].tolist()
    rects = SamplePrep.window(2, 24, 40, (fh, fw), np.random.RandomState(int(fixture["mask_seed"])))
    assert rects.dtype == np.int32 and rects.shape == (2, 4) and (rects[0] == rects[1]).all() and tuple(rects[0, 2:]) == (fh, fw)
    mask = P.window_mask(rects[0], 24, 40, torch.float32)
    assert torch.equal(mask, fixture["mask"].float()) and int((mask == 0).sum()) == fh * fw
    img = fixture["center32"][:2].permute(0, 3, 1, 2)
    assert float((img * mask).double().sum()) == pytest.approx(float(fixture["masked_sum"]), rel=1e-12)
    assert (SamplePrep.window(2, 24, 40, (24, 40), np.random.RandomState(1)) == 0).all()       # the whole image: no window


# ---- the restatement against PIL and colorsys ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pil_image():
    u8 = P.seeded_views(1, 37, 53, 611)[0]
    flat = u8.view(-1, 3)
    assert all(bool((flat == v).all(1).any()) for v in (0, 255, 128))          # black, white and grey pixels
    return u8


@pytest.mark.parametrize("f", [0, 0.3, 0.77, 1, 1.4, 2])
@pytest.mark.parametrize("op", ["brightness", "contrast", "saturation"])
def test_oracle_vs_pil_image_enhance(pil_image, op, f):
    """One operation at a time against PIL.ImageEnhance, which truncates to uint8 and takes the contrast mean / the grey image
    integer-rounded: brightness within 1 level of 255, contrast and saturation within 2."""
    from PIL import Image, ImageEnhance
    enh = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}[op]
    want = torch.from_numpy(np.array(enh(Image.fromarray(pil_image.numpy(), "RGB")).enhance(f))).double()
    got = getattr(P, op)(pil_image.double() / 255, torch.tensor(float(f), dtype=torch.float64)) * 255
    diff = float((got - want).abs().max())
    print("%s f = %g: max difference %.3f levels" % (op, f, diff))
    assert diff < (1.0 if op == "brightness" else 2.0)


def test_oracle_hue_vs_colorsys(pil_image):
    """hue, pixel by pixel, against colorsys.rgb_to_hsv / hsv_to_rgb with h = (h + f) % 1: grey, saturated and ordinary pixels,
    shifts of +-0.5 among them, to 1e-12."""
    x = pil_image.double().view(-1, 3) / 255
    extra = torch.tensor([[0.2, 0.2, 0.2], [1.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.5, 0.5, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                         dtype=torch.float64)
    x = torch.cat([extra, x[::3]], 0)
    for f in (0.5, -0.5, 0.0, 0.13, -0.37):
        got = P.hue(x, torch.tensor(f, dtype=torch.float64))
        for i in range(x.shape[0]):
            r, g, b = x[i].tolist()
            h, s, v = colorsys.rgb_to_hsv(r, g, b)
            want = colorsys.hsv_to_rgb((h + f) % 1.0, s, v)
            assert max(abs(a - w) for a, w in zip(got[i].tolist(), want)) <= 1e-12, (f, i, x[i].tolist(), got[i].tolist(), want)
    grey = P.hue(extra[:1], torch.tensor(0.3, dtype=torch.float64))
    assert torch.equal(grey, extra[:1])


# ---- the emulated kernels against the restatement -----------------------------------------------------------------------------------

def _oracles(used, table, rects, **kw):
    return P.prepare(used.contiguous(), table, rects, torch.float32, **kw), P.prepare(used.contiguous(), table, rects, torch.float64, **kw)


def test_cases_cover_what_they_claim():
    """every one of the 24 operation orders, absent operations, gamma 0.5 / 1 / 2, hue shifts of exactly +-0.5, a window on the
    first view of each sample, and sizes that are no multiple of 4 / 16 / the tile"""
    orders, gammas, absent, hues = set(), set(), 0, set()
    for name in P.CASES:
        stored, used, table, rects = P.make_case(name)
        M, H, W, rows, N = P.CASES[name]
        assert tuple(used.shape) == (M, rows, W, 3) and table.shape == (M, 9) and rects.shape == (M, 4)
        for m in range(M):
            ids = tuple(int(v) for v in table[m, :4])
            if -1 in ids:
                absent += 1
            else:
                orders.add(ids)
                hues.add(float(table[m, 4 + ids.index(3)]))
            gammas.add(float(table[m, 8]))
            assert (rects[m, 2] > 0) == (m % N == 0 and rows // 3 > 0)
    assert orders == set(P.ORDERS) and absent >= 3 and {0.5, 1.0, 2.0} <= gammas and {0.5, -0.5} <= hues
    assert (37 * 53) % 4 and (37 * 53 * 3) % 16 and 37 % 4 and 53 % 4 and 1030 % 16 and (130 * 1030) % 4096 and 5 * 7 < 4096
    assert not P.make_case("crop")[1].is_contiguous()


@pytest.mark.parametrize("name", list(P.CASES))
def test_emulated_kernels_vs_oracle(emul_lib, name):
    """ops.sample_prep through the emulated kernels on the shapes of the GPU test, by the criteria of the issue; three launches;
    a second run gives the same bits; the channels-last outputs are equal element by element; the views are not modified."""
    from mvs_amd import ops
    stored, used, table, rects = P.make_case(name)
    keep = stored.clone()
    o32, o64 = _oracles(used, table, rects, mask_scale=4)
    emul_lib.launch_trace()
    out = ops.sample_prep(used, table, rects, mask_scale=4)
    assert emul_lib.launch_trace() == ["sample_prep_stats", "sample_prep_aug_stats", "sample_prep_write"]
    assert torch.equal(stored, keep)
    P.check_outputs(out, o32, o64, what=name)
    if name in ("odd", "crop", "tiny"):
        again = ops.sample_prep(used, table, rects, mask_scale=4)
        cl = ops.sample_prep(used, table, rects, mask_scale=4, channels_last=True)
        for k, v in out.items():
            assert torch.equal(again[k], v), k
            assert torch.equal(cl[k], v), k
            if k != "filter_mask":
                assert cl[k].permute(0, 2, 3, 1).is_contiguous() and v.is_contiguous()


def test_emulated_without_table_and_full_size_mask(emul_lib):
    """No table: two launches, no imgs_aug, the other outputs unchanged; mask_scale 1 is the window itself; single outputs."""
    from mvs_amd import ops
    stored, used, table, rects = P.make_case("odd")
    full = ops.sample_prep(used, table, rects, mask_scale=4)
    emul_lib.launch_trace()
    out = ops.sample_prep(used, None, rects, mask_scale=1)
    assert emul_lib.launch_trace() == ["sample_prep_stats", "sample_prep_write"]
    assert sorted(out) == ["filter_mask", "imgs", "imgs_seg"]
    assert torch.equal(out["imgs"], full["imgs"]) and torch.equal(out["imgs_seg"], full["imgs_seg"])
    for m in range(3):
        assert torch.equal(out["filter_mask"][m], P.window_mask(rects[m], 37, 53, torch.float32))
    only = ops.sample_prep(used, table, None, imgs=False, seg=False)
    assert sorted(only) == ["imgs_aug"]
    o64 = P.prepare(used, table, None, torch.float64)
    o32 = P.prepare(used, table, None, torch.float32)
    assert_as_accurate_as_fp32_reference(only["imgs_aug"], o32["imgs_aug"], o64["imgs_aug"], what="no window")
    seg = ops.sample_prep(used, None, None, imgs=False, seg=True)
    assert sorted(seg) == ["imgs_seg"] and torch.equal(seg["imgs_seg"], full["imgs_seg"])
    assert emul_lib.launch_trace()[-1:] == ["sample_prep_write"]


def test_emulated_more_views_than_one_group_of_launches(emul_lib):
    """70 views of 6 x 10: the parameters of 64 views travel in one group of launches, so this takes two groups (six launches);
    every view still gets its own order, factors, gamma and window."""
    from mvs_amd import ops
    views = P.seeded_views(70, 6, 10, 631)
    table = P.seeded_table(70, 632, first_order=3, gammas=())
    low = (table[:, :4] <= 1) & (table[:, 4:8] < 0.5)         # brightness / contrast factors near 0 leave a nearly constant view,
    table[:, 4:8][low] = 0.5                                  # whose centring divides by ~0: ill-conditioned for every evaluation
    rects = np.zeros((70, 4), np.int32)
    rects[::7] = (1, 2, 1, 2)
    o32, o64 = _oracles(views, table, rects, mask_scale=1)
    emul_lib.launch_trace()
    out = ops.sample_prep(views, table, rects, mask_scale=1)
    assert emul_lib.launch_trace() == ["sample_prep_stats", "sample_prep_aug_stats", "sample_prep_write"] * 2
    P.check_outputs(out, o32, o64, what="70 views")


def test_emulated_augmentor_form(emul_lib):
    """src_kind 1: fp32 [2 * 3, 3, 36, 52] in [0, 1], quantised on load, brightness and contrast only, no centring, an (h // 4,
    w // 4) window on each sample's first view, the full-size mask: two launches."""
    from mvs_amd import ops
    x, table, rects = P.augmentor_case()
    u8 = P.quantise(x)
    assert torch.equal(u8, P.quantise(x.double())) and int((u8 == 0).sum()) > 0 and int((u8 == 255).sum()) > 0
    o32 = P.prepare(u8, table, rects, torch.float32, aug_center=False, mask_scale=1)
    o64 = P.prepare(u8, table, rects, torch.float64, aug_center=False, mask_scale=1)
    emul_lib.launch_trace()
    out = ops.sample_prep(x, table, rects, imgs=False, seg=False, mask_scale=1, aug_center=False)
    assert emul_lib.launch_trace() == ["sample_prep_stats", "sample_prep_write"]
    want = {k: o64[k] for k in ("imgs_aug", "filter_mask")}
    P.check_outputs(out, o32, want, what="augmentor")
    assert float(out["imgs_aug"].min()) >= 0.0 and float(out["imgs_aug"].max()) <= 1.0
    assert int((out["filter_mask"][0] == 0).sum()) == 9 * 13 and bool((out["filter_mask"][1] == 1).all())


def test_sample_prep_class_and_augmentor_through_the_emulation(emul_lib):
    """SamplePrep()(views [B, N, H, W, 3], table, rects) returns the tensors train_sample consumes, equal to the flat call;
    Augmentor shares one jitter draw among a sample's views, draws a gamma per view, and returns the [B, 3, H, W] mask."""
    from mvs_amd import ops
    from mvs_amd.sample_prep import SamplePrep
    from mvs_amd.jdacs.models import augmentations as A
    from mvs_amd.jdacs_ms.models import augmentations as A2
    assert A2.Augmentor is A.Augmentor and A2.RandomGamma is A.RandomGamma and A2.get_transform is A.get_transform
    B, N, H, W = 2, 3, 20, 28
    views = P.seeded_views(B * N, H, W, 621).view(B, N, H, W, 3)
    prep = SamplePrep()
    rs = np.random.RandomState(3)
    table, rects = prep.draw(B * N, rs), prep.window(B, H, W, (H // 3, W // 3), rs)
    out = prep(views, table, rects)
    assert sorted(out) == ["filter_mask", "imgs", "imgs_aug", "imgs_seg"]
    assert all(tuple(out[k].shape) == (B, N, 3, H, W) for k in ("imgs", "imgs_aug", "imgs_seg"))
    assert tuple(out["filter_mask"].shape) == (B, H // 4, W // 4)
    flat_rects = np.zeros((B, N, 4), np.int32)
    flat_rects[:, 0] = rects
    flat = ops.sample_prep(views.view(B * N, H, W, 3), table, flat_rects.reshape(-1, 4), mask_scale=4)
    for k in ("imgs", "imgs_aug", "imgs_seg"):
        assert torch.equal(out[k].reshape(B * N, 3, H, W), flat[k]), k
    assert torch.equal(out["filter_mask"], flat["filter_mask"].view(B, N, H // 4, W // 4)[:, 0])
    y, x, fh, fw = rects[0]
    assert bool((out["imgs_aug"][:, 0, :, y:y + fh, x:x + fw] == 0).all()) and bool((out["imgs_aug"][:, 1, :, y:y + fh, x:x + fw] != 0).any())
    cropped = prep(views, None, None, rows=16)
    assert sorted(cropped) == ["imgs", "imgs_seg"] and tuple(cropped["imgs"].shape) == (B, N, 3, 16, W)
    assert torch.equal(cropped["imgs_seg"], out["imgs_seg"][:, :, :, :16])

    x01 = ((views.float() + 0.5) / 255).clamp(0, 1).permute(0, 1, 4, 2, 3).contiguous()
    aug = A.Augmentor()
    np.random.seed(77)
    got, mask = aug(x01)
    np.random.seed(77)
    table = aug.transform.draw(B, N)
    win = SamplePrep.window(B, H, W, (H // 4, W // 4), np.random.mtrand._rand)
    assert tuple(got.shape) == (B, N, 3, H, W) and tuple(mask.shape) == (B, 3, H, W)
    for b in range(B):
        assert (table[b * N:(b + 1) * N, :8] == table[b * N, :8]).all()                 # one jitter draw per sample
        assert len(set(table[b * N:(b + 1) * N, 8].tolist())) == N                      # a gamma per view
        assert sorted(table[b * N, :4].tolist()) == [-1, -1, 0, 1]                      # brightness and contrast only
    assert not (table[0, :8] == table[N, :8]).all()
    assert bool((0.7 <= table[:, 8]).all()) and bool((table[:, 8] <= 2.0).all())
    flat_rects[:, 0] = win
    want = P.prepare(P.quantise(x01.view(B * N, 3, H, W)), table, flat_rects.reshape(-1, 4), torch.float64, aug_center=False,
                     mask_scale=1)
    assert float((got.reshape(B * N, 3, H, W).double() - want["imgs_aug"]).abs().max()) < 1e-5
    assert torch.equal(mask[:, 0], want["filter_mask"].float().view(B, N, H, W)[:, 0]) and torch.equal(mask[:, 0], mask[:, 2])
    one = A.get_transform()(list(x01[0]))
    assert len(one) == N and tuple(one[0].shape) == (3, H, W)
    assert A.RandomGamma.adjust_gamma(torch.tensor([0.25, 2.0]), 0.5, True).tolist() == [0.5, 1.0]
    assert 0.7 <= A.RandomGamma.get_params(0.7, 1.5) <= 1.5


# ---- the parameter draws ------------------------------------------------------------------------------------------------------------

RECORDED = [        # SamplePrep().draw(3, RandomState(5)): ids in application order, their factors, gamma
    [2.0, 1.0, 3.0, 0.0, 0.706719160079956, 1.741464614868164, 0.41861090064048767, 0.44398635625839233, 1.0951049327850342],
    [2.0, 1.0, 0.0, 3.0, 1.4908208847045898, 0.9732760190963745, 0.708276093006134, 0.30828168988227844, 1.1619638204574585],
    [0.0, 3.0, 1.0, 2.0, 0.31661972403526306, -0.08576498180627823, 1.7598741054534912, 0.7740864753723145, 1.285512924194336]]


def test_draw_reproduces_a_recorded_table():
    from mvs_amd.sample_prep import SamplePrep
    table = SamplePrep().draw(3, np.random.RandomState(5))
    assert table.dtype == np.float32 and table.shape == (3, 9)
    assert np.array_equal(table, np.asarray(RECORDED, np.float32)), table.tolist()


def test_draw_ranges_orders_and_absent_operations():
    """10 000 draws: every factor inside its range and the ranges used up to their ends, each of the 24 orders occurs, gamma in its
    range; a zero setting removes the operation (-1 behind the present ones, factor 1)."""
    from mvs_amd.sample_prep import SamplePrep
    t = SamplePrep().draw(10000, np.random.RandomState(11))
    ids = t[:, :4].astype(int)
    assert (np.sort(ids, 1) == np.arange(4)).all()
    assert {tuple(r) for r in ids.tolist()} == set(P.ORDERS)
    lo, hi = np.asarray([0.0, 0.0, 0.5, -0.5]), np.asarray([2.0, 2.0, 1.5, 0.5])
    f = np.take_along_axis(t[:, 4:8], np.argsort(ids, 1), 1)                  # factors by operation
    assert (f >= lo).all() and (f <= hi).all() and (f.min(0) < lo + 0.01).all() and (f.max(0) > hi - 0.01).all()
    assert (t[:, 8] >= 0.5).all() and (t[:, 8] <= 2.0).all() and t[:, 8].min() < 0.51 and t[:, 8].max() > 1.99
    t = SamplePrep(brightness=0.5, contrast=0.5, saturation=0, hue=0, gamma=(0.7, 2.0)).draw(2000, np.random.RandomState(12))
    assert (np.sort(t[:, :2].astype(int), 1) == [0, 1]).all() and (t[:, 2:4] == -1).all() and (t[:, 6:8] == 1).all()
    assert (t[:, 4:6] >= 0.5).all() and (t[:, 4:6] <= 1.5).all() and t[:, 8].min() >= 0.7
    assert {tuple(r) for r in t[:, :2].astype(int).tolist()} == {(0, 1), (1, 0)}
    t = SamplePrep(brightness=3).draw(500, np.random.RandomState(13))             # [max(0, 1 - 3), 1 + 3]
    f = t[:, 4:8][t[:, :4] == 0]
    assert f.min() >= 0.0 and f.max() <= 4.0 and f.max() > 3.5
    with pytest.raises(ValueError):
        SamplePrep(hue=0.6)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------

def _product_lib():
    from mvs_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.MvsLib()


def test_entry_point_rejects_bad_arguments():
    """mvs_sample_prep on the product library without a GPU: every bad argument returns its negative code with a message before
    anything is launched; the workspace query answers -1 for the same sizes and M * ceil(H W / 4096) * 128 otherwise."""
    lib = _product_lib()
    d = C.c_void_p(64)                      # never dereferenced
    good = [0, 1, 2, 3, 1.5, 0.5, 1.2, 0.25, 0.8]

    def call(src=d, kind=0, stride=0, rows=(good, good), rect=None, imgs=d, aug=d, seg=d, fm=d, scale=4, m=2, h=10, w=12, ws=d):
        tab = None if rows is None else (C.c_float * (9 * len(rows)))(*[v for r in rows for v in r])
        rec = None if rect is None else (C.c_int * (4 * len(rect)))(*[v for r in rect for v in r])
        return lib.raw("mvs_sample_prep", src, kind, stride, tab, rec, imgs, aug, seg, fm, scale, 1, 0, m, h, w, ws, None)

    lib.launch_trace()
    cases = [
        (dict(m=0), -1, "M, H, W >= 1"), (dict(h=0), -1, "M, H, W >= 1"), (dict(w=-3), -1, "M, H, W >= 1"),
        (dict(m=1, h=26755, w=26755, rows=(good,)), -1, "below 2\\^31"),
        (dict(ws=None), -4, "null pointer"), (dict(src=None), -4, "null pointer"),
        (dict(imgs=None, aug=None, seg=None, fm=None), -4, "every output"),
        (dict(rows=None), -4, "needs the parameter table"),
        (dict(kind=2), -2, "src_kind"), (dict(scale=3), -2, "mask_scale 1 or 4"), (dict(stride=100), -1, "image stride"),
        (dict(rows=(good, [0, 1, 2, 4] + good[4:])), -2, "bad operation id 4"),
        (dict(rows=(good, [0, 1.5, 2, 3] + good[4:])), -2, "bad operation id 1.5"),
        (dict(rows=([-2, 1, 2, 3] + good[4:], good)), -2, "bad operation id -2"),
        (dict(rows=(good, [0, 1, 1, 3] + good[4:])), -2, "twice"),
        (dict(rows=(good, good[:8] + [0.0])), -2, "gamma"), (dict(rows=(good, good[:8] + [float("nan")])), -2, "gamma"),
        (dict(rows=(good, good[:4] + [float("inf")] + good[5:])), -2, "not finite"),
        (dict(rect=((0, 0, 0, 0), (8, 0, 3, 3))), -1, "leaves the 10 x 12 image"),
        (dict(rect=((0, 0, 0, 0), (0, -1, 3, 3))), -1, "leaves the"),
    ]
    import re
    for kw, code, msg in cases:
        assert call(**kw) == code, kw
        assert re.search(msg, lib.raw("mvs_last_error").decode()), (kw, lib.raw("mvs_last_error"))
    with pytest.raises(ValueError, match="null pointer"):            # the wrapper's checked call raises on a negative code
        lib.call("mvs_sample_prep", None, 0, 0, None, None, d, None, None, None, 4, 1, 0, 2, 10, 12, d, None)
    for m, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 26755, 26755), (3, 20000, 20000)):
        assert lib.raw("mvs_sample_prep_workspace_bytes", m, h, w) == -1
    for m, h, w in ((1, 1, 1), (1, 5, 7), (3, 37, 53), (5, 128, 160), (2, 130, 1030), (5, 1184, 1600), (3, 64, 64), (1, 4097, 1)):
        assert lib.raw("mvs_sample_prep_workspace_bytes", m, h, w) == m * ((h * w + 4095) // 4096) * 128
    assert lib.launch_trace() == []


def test_wrapper_rejects_what_it_cannot_serve(emul_lib, monkeypatch):
    from mvs_amd import _lib, ops
    stored, used, table, rects = P.make_case("tiny")
    with pytest.raises(TypeError, match="uint8 .* or float32"):
        ops.sample_prep(used.double(), table)
    with pytest.raises(ValueError, match=r"\[M,H,W,3\]"):
        ops.sample_prep(used.permute(0, 3, 1, 2), table)
    with pytest.raises(ValueError, match="table must be"):
        ops.sample_prep(used, table[:, :8])
    with pytest.raises(ValueError, match="rects must be"):
        ops.sample_prep(used, table, np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="mask_scale"):
        ops.sample_prep(used, table, mask_scale=2)
    with pytest.raises(ValueError, match="no output"):
        ops.sample_prep(used, None, imgs=False, seg=False)
    bad = table.copy()
    bad[0, 2] = 7
    with pytest.raises(ValueError, match="bad operation id 7"):
        ops.sample_prep(used, bad)
    _product_lib()
    monkeypatch.setattr(_lib, "_INSTANCE", None)         # the next ops call loads the product library
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_prep(used, table)


def test_source_enqueues_only_and_has_no_atomics():
    """csrc/sample_prep_kernels.h holds no stream / device / event synchronisation, no copy and no atomics: three enqueued
    launches, sums through LDS and tile records in a fixed order; loss.hip includes it."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "self-supervised-mvs_amd", "csrc", "sample_prep_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("Synchronize", "hipMemcpy", "hipStreamQuery", "hipEventQuery", "hipHostMalloc", "hipStreamWaitEvent", "atomic",
                 "ATOMIC", "volatile", "__threadfence", "while ("):
        assert word not in code, word
    assert code.count("MVS_LAUNCH(") == 3
    assert "sample_prep_kernels.h" in open(os.path.join(root, "self-supervised-mvs_amd", "csrc", "loss.hip")).read()
