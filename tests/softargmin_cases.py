"""TEST INFRASTRUCTURE: inputs of the soft-argmin size-switch cases (csrc/softargmin.hip: D < 32 one lane group per pixel; 32 <= D <=
256 four lane groups with the logits in registers; D > 256 four lane groups re-reading memory), shared by the emulation test and
the GPU test.  The confidence window is indexed by trunc(E[d]): a pixel whose expectation sits on an integer may flip legitimately,
so every case carries a seed for which the float64 reference has NO pixel with E[d] within 1e-3 of an integer -- asserted on the
inputs, so that no pixel is excluded from the comparison."""
import torch

from oracle import ref_torch as R

# (D, (H, W), per-pixel hypotheses, seed): D either side of both switches and with unequal work for the four lane groups (33, 131,
# 257); H * W is never a multiple of the 16 pixels of a wave
CASES = [(d, (5, 7) if i % 2 == 0 else (3, 11), pp, 0) for i, d in enumerate((32, 33, 131, 256, 257, 300)) for pp in (False, True)]
IDS = ["D%d_%s_%dx%d" % (d, "per_pixel" if pp else "fixed", hw[0], hw[1]) for d, hw, pp, _ in CASES]


def inputs(d, hw, per_pixel, seed, b=2):
    gen = torch.Generator().manual_seed(1000 * d + 10 * hw[1] + seed)
    h, w = hw
    lg = torch.randn(b, d, h, w, generator=gen) * 3
    hyp = 500 + torch.rand(b, d, h, w, generator=gen) * 50 if per_pixel else (425 + 7.0 * torch.arange(d)).unsqueeze(0).repeat(b, 1)
    gd = torch.randn(b, h, w, generator=gen)
    return lg, hyp, gd


def margin(lg):
    """smallest distance of the float64 expectation E[d] of any pixel from an integer"""
    e = (torch.softmax(lg.double(), dim=1) * torch.arange(lg.shape[1], dtype=torch.float64).view(1, -1, 1, 1)).sum(1)
    return float((e - e.round()).abs().min())


def reference64(lg, hyp, gd):
    """depth, confidence and d depth / d logits of oracle.ref_torch.softargmin_conf in float64"""
    lg64 = lg.double().requires_grad_(True)
    dep, conf, _ = R.softargmin_conf(lg64, hyp.double())
    dep.backward(gd.double())
    return dep.detach(), conf.detach(), lg64.grad


def check(dep, conf, glg, lg, hyp, gd):
    """the tolerances of test_softargmin_smallest_shapes, against the float64 reference"""
    assert margin(lg) > 1e-3, "pick another seed: a pixel's E[d] is within 1e-3 of an integer (%.2e)" % margin(lg)
    e, ec, eg = reference64(lg, hyp, gd)
    print("softargmin D=%d: depth err %.3e conf err %.3e grad err %.3e (|g| max %.3e)" % (
        lg.shape[1], float((dep.double() - e).abs().max()), float((conf.double() - ec).abs().max()),
        float((glg.double() - eg).abs().max()), float(eg.abs().max())))
    assert float((dep.double() - e).abs().max()) < 1e-3
    assert float((conf.double() - ec).abs().max()) < 1e-5
    assert float((glg.double() - eg).abs().max()) < 1e-4 * max(1.0, float(eg.abs().max()))
