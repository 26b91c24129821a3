"""Drop-in for jdacs/models/seg_dff.py: ``NMF(V, k, ...)`` and ``SegDFF(K, max_iter)(imgs)``.

Same call signatures and return values as the reference (seg_dff.py:50-143).  The multiplicative-update solver -- a dozen small
launches per iteration and a host synchronisation at every tenth one in the reference -- is one ``ops.nmf_solve`` call for the
whole batch (csrc/seg_loss_kernels.h: two launches per iteration, the stopping decision taken on the device) and its status is
read back once per batch.  The feature extractor stays a stock PyTorch call: a frozen, pretrained third-party network under
``no_grad``, not part of this path.

Differences from the reference, on purpose: the initial factors come from a private ``torch.Generator``
(the reference re-seeds the global generator and then restores the *initial* seed, a side effect not copied); a solve whose W
holds a non-finite value is repeated with a fresh seed at most ``MAX_ATTEMPTS`` times (the reference retries without limit)."""
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

MAX_ATTEMPTS = 4


def initial_factors(V, k, seed=None):
    """|randn| * sqrt(mean(V) / k) for W [..,n,k] and then H [..,k,m] (seg_dff.py:55-89), drawn on V's device from a private
    generator seeded with ``seed`` (None: the device's global generator, as the reference does without a seed)."""
    gen = None
    if seed is not None:
        gen = torch.Generator(device=V.device)
        gen.manual_seed(int(seed))
    n, m = V.shape[-2:]
    scale = torch.sqrt(V.mean() / k)
    W = torch.randn(n, k, generator=gen, device=V.device, dtype=V.dtype) * scale
    H = torch.randn(k, m, generator=gen, device=V.device, dtype=V.dtype) * scale
    return torch.abs(W), torch.abs(H)


def NMF(V, k, W=None, H=None, random_seed=None, max_iter=200, tol=1e-4, cuda=True, verbose=False):
    """V [n,m] >= 0 -> (W [n,k], H [k,m]).  A caller-supplied H stays fixed (only W is updated), as in the reference."""
    update_h = H is None
    if W is None or H is None:
        W0, H0 = initial_factors(V, k, random_seed)      # W is drawn before H
        W = W0 if W is None else W
        H = H0 if H is None else H
    W, H = torch.abs(W), torch.abs(H)
    Wr, Hr, status = ops.nmf_solve(V, W, H, update_h=update_h, max_iter=max_iter, tol=tol)
    if verbose:
        print("Exited after {} iterations.".format(int(status[0, 0])))
    return Wr, Hr


class SegDFF(nn.Module):
    """imgs [B,N,3,H,W] -> heatmaps [B,N,h,w,K] (requires_grad False): deep feature factorisation of the frozen network's
    features, one NMF problem per batch item (seg_dff.py:109-143).  net: the feature extractor (its ``.features`` is applied
    to the 224x224 images); None = torchvision's pretrained VGG19 without ``features['36']``, as in the reference."""

    def __init__(self, K, max_iter=50, net=None):
        super().__init__()
        self.K = K
        self.max_iter = max_iter
        if net is None:
            try:
                from torchvision import models
            except ImportError as exc:
                raise ImportError("SegDFF needs torchvision for its pretrained VGG19 feature extractor (or pass net=...): "
                                  "torchvision cannot be imported (%s)" % exc) from exc
            net = models.vgg19(pretrained=True)
            del net.features._modules['36']  # the last pooling layer is not used
        self.net = net

    def _solve(self, flat, seeds):
        """flat [P,n,m], one seed per problem -> W [P,n,K], status [P,4]: one kernel call for all problems"""
        facs = [initial_factors(flat[i], self.K, s) for i, s in enumerate(seeds)]
        W0 = torch.stack([f[0] for f in facs])
        H0 = torch.stack([f[1] for f in facs])
        W, _, status = ops.nmf_solve(flat, W0, H0, update_h=True, max_iter=self.max_iter, tol=1e-4)
        return W, status

    def forward(self, imgs):
        b, nv = imgs.shape[:2]
        with torch.no_grad():
            x = F.interpolate(imgs.reshape(b * nv, *imgs.shape[2:]), size=(224, 224), mode='bilinear', align_corners=False)
            features = self.net.features(x)
            c, h, w = features.shape[1:]
            flat = features.permute(0, 2, 3, 1).reshape(b, nv * h * w, c).float().contiguous()
            W, status = self._solve(flat, [1] * b)
            bad = (status[:, 1] > 0).nonzero().flatten().tolist()     # the one status read of the batch
            attempt = 1
            while bad:
                # NMF sometimes fails (W all NaN, useless in the backward pass): solve those items again from other random factors
                if attempt >= MAX_ATTEMPTS:
                    raise RuntimeError("SegDFF: the NMF of batch item(s) %s still holds non-finite values after %d attempts"
                                       % (bad, MAX_ATTEMPTS))
                print('nan detected. trying to resolve the nmf.')
                Wb, sb = self._solve(flat[bad], [random.randint(0, 255) for _ in bad])
                W[bad] = Wb
                bad = [bad[i] for i in (sb[:, 1] > 0).nonzero().flatten().tolist()]
                attempt += 1
            heatmaps = W.view(b, nv, h, w, self.K)
        heatmaps.requires_grad = False
        return heatmaps
