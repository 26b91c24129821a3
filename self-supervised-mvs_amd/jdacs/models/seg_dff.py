"""Drop-in for jdacs/models/seg_dff.py: ``NMF(V, k, ...)`` and ``SegDFF(K, max_iter)(imgs)``.

Same call signatures and return values as the reference (seg_dff.py:50-143).  The multiplicative-update solver -- a dozen small
launches per iteration and a host synchronisation at every tenth one in the reference -- is one ``ops.nmf_solve`` call for the
whole batch (csrc/seg_loss_kernels.h: two launches per iteration, the stopping decision taken on the device) and its status is
read back once per batch.  The feature extractor -- a frozen network under ``no_grad`` -- has two routes: the stock PyTorch
call (``F.interpolate`` + ``net.features`` + a layout change), and, for a trunk of 3x3 convolutions, ReLUs and 2x2 max pools
(``trunk_served``: VGG19's shape), the HIP route ``ops.resize_bilinear_cl`` + ``ops.conv_trunk_forward``
(csrc/conv2d_wide_kernels.h), whose last output already is the matrix the NMF reads.  ``SegDFF(hip_features=...)`` chooses;
DESIGN.md section 7 has the measurement behind the default.  ``vgg19_trunk(state_dict)`` builds VGG19's feature trunk with
torchvision's parameter names without torchvision.

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


# VGG19's feature trunk (Simonyan & Zisserman 2015, configuration E): output channels of the 3x3 convolutions, "M" = 2x2 max pool.
# The last pool of the published table is left out, as SegDFF does not use it.
VGG19_LAYERS = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512)


class _Trunk(nn.Module):
    def __init__(self, features):
        super().__init__()
        self.features = features

    def forward(self, x):
        return self.features(x)


def conv_trunk(layers, in_channels=3):
    """``.features`` = nn.Sequential of Conv2d(3x3, pad 1) + ReLU per number and MaxPool2d(2, 2) per "M" of ``layers``, initialised as
    torchvision initialises VGG (kaiming_normal_(fan_out, relu), bias 0), parameters frozen."""
    mods, cin = [], in_channels
    for v in layers:
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            conv = nn.Conv2d(cin, v, kernel_size=3, padding=1)
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(conv.bias, 0)
            mods += [conv, nn.ReLU(inplace=True)]
            cin = v
    net = _Trunk(nn.Sequential(*mods))
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def vgg19_trunk(state_dict=None):
    """VGG19's feature extractor without its last pool, built here (no torchvision): ``.features`` has torchvision's indices --
    convolutions at 0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34, each followed by a ReLU, MaxPool2d(2, 2) at 4, 9,
    18, 27, no entry 36 -- so a VGG19 weight file a user already has loads without renaming: ``state_dict`` may be the whole
    model's (``features.*`` are taken, the classifier's and ``features.36``-less extras ignored) or just the trunk's.  Without
    one the weights are random (torchvision's initialisation); nothing is downloaded."""
    net = conv_trunk(VGG19_LAYERS)
    if state_dict is not None:
        own = net.state_dict()
        picked = {k: v for k, v in state_dict.items() if k in own}
        missing = sorted(set(own) - set(picked))
        if missing:
            raise KeyError("vgg19_trunk: the state dict lacks %s" % ", ".join(missing))
        net.load_state_dict(picked)
    return net.eval()


def trunk_layers(net):
    """[(Conv2d, relu, pool_after)] when ``net.features`` is an nn.Sequential the HIP trunk serves, else None: only Conv2d (3x3,
    stride 1, padding 1, dilation 1, groups 1, zeros padding, 3 or 32..512 input and 32..512 output channels in steps of 32),
    each optionally followed directly by a ReLU, and MaxPool2d(2, 2, ceil_mode=False) directly after a ReLU."""
    feats = getattr(net, "features", None)
    if not isinstance(feats, nn.Sequential) or len(feats) == 0:
        return None
    mods, layers, i = list(feats), [], 0
    while i < len(mods):
        m = mods[i]
        if type(m) is not nn.Conv2d:
            return None
        if (tuple(m.kernel_size), tuple(m.stride), tuple(m.dilation), m.groups, m.padding_mode) != ((3, 3), (1, 1), (1, 1), 1, "zeros") \
                or m.padding not in ((1, 1), 1, "same") or not ops.conv2d_wide_serves(m.in_channels, m.out_channels) \
                or m.weight.dtype != torch.float32:
            return None
        i += 1
        relu = i < len(mods) and type(mods[i]) is nn.ReLU
        i += relu
        pool = False
        if relu and i < len(mods) and type(mods[i]) is nn.MaxPool2d:
            p = mods[i]
            two = lambda v: v in (2, (2, 2))
            if not (two(p.kernel_size) and two(p.stride) and p.padding in (0, (0, 0)) and p.dilation in (1, (1, 1)) and not p.ceil_mode
                    and not p.return_indices):
                return None
            pool = True
            i += 1
        layers.append((m, relu, pool))
    if any(a[0].out_channels != b[0].in_channels for a, b in zip(layers, layers[1:])):
        return None
    return layers


def trunk_served(net):
    """True when ``net.features`` can run on the HIP trunk (``trunk_layers``)."""
    return trunk_layers(net) is not None


class SegDFF(nn.Module):
    """imgs [B,N,3,H,W] -> heatmaps [B,N,h,w,K] (requires_grad False): deep feature factorisation of the frozen network's
    features, one NMF problem per batch item (seg_dff.py:109-143).  net: the feature extractor (its ``.features`` is applied
    to the 224x224 images); None = torchvision's pretrained VGG19 without ``features['36']``, as in the reference.
    hip_features: False = the stock PyTorch call; True = the HIP trunk (raises when ``trunk_served(net)`` is false); None = the
    HIP trunk when it is served, the images are on the GPU and HIP_FEATURES_DEFAULT says so.
    feature_arith: the arithmetic of the HIP trunk's multiplications (``ops.conv2d_wide_forward``): "f32" (default) or "bf16";
    opt-in.  Anything but "f32" means the HIP trunk (as ``hip_features=True``: there is no such stock path), so it is
    a ValueError together with ``hip_features=False`` or with a network the HIP trunk does not serve."""

    # what ``hip_features=None`` does with a served trunk on the GPU: set by the measurement of tools/vgg_features_bench.py
    # (profiles/vgg_features_timing.json) under the rule "HIP only when its p90 is below the stock path's p10": N = 7 on one
    # MI355X, HIP 3.088 ms (p90 3.104) against 3.182 ms (p10 3.168) for the stock path
    HIP_FEATURES_DEFAULT = True

    def __init__(self, K, max_iter=50, net=None, hip_features=None, feature_arith="f32"):
        super().__init__()
        ops.wide_arith(feature_arith)
        if feature_arith not in (0, "f32") and hip_features is False:
            raise ValueError("SegDFF(feature_arith=%r) is an arithmetic of the HIP trunk: it cannot go with hip_features=False" % (feature_arith,))
        self.K = K
        self.max_iter = max_iter
        if net is None:
            try:
                from torchvision import models
            except ImportError as exc:
                raise ImportError("SegDFF needs torchvision for its pretrained VGG19 feature extractor: torchvision cannot be "
                                  "imported (%s).  Without torchvision pass net=vgg19_trunk(state_dict=...) with a VGG19 weight "
                                  "file of your own (torchvision's key names), or any other net=..." % exc) from exc
            net = models.vgg19(pretrained=True)
            del net.features._modules['36']  # the last pooling layer is not used
        self.net = net
        if hip_features and not trunk_served(net):
            raise ValueError("SegDFF(hip_features=True): net.features is not a trunk the HIP kernels serve (3x3 stride-1 pad-1 "
                             "convolutions with 3 or 32..512 -> 32..512 channels in steps of 32, ReLU, MaxPool2d(2, 2))")
        if feature_arith not in (0, "f32"):
            if not trunk_served(net):
                raise ValueError("SegDFF(feature_arith=%r): net.features is not a trunk the HIP kernels serve" % (feature_arith,))
            hip_features = True
        self.hip_features = hip_features
        self.feature_arith = feature_arith

    def _hip_route(self, imgs):
        if self.hip_features is False:
            return None
        if self.hip_features is None and not (self.HIP_FEATURES_DEFAULT and imgs.is_cuda):
            return None
        layers = trunk_layers(self.net)
        if layers is None:
            if self.hip_features:
                raise ValueError("SegDFF(hip_features=True): net.features is no longer a trunk the HIP kernels serve")
            return None
        return layers

    def _features(self, imgs):
        """imgs [B,N,3,H,W] -> (flat [B, N h w, C], h, w)"""
        b, nv = imgs.shape[:2]
        x = imgs.reshape(b * nv, *imgs.shape[2:])
        layers = self._hip_route(imgs)
        if layers is not None:
            x = ops.resize_bilinear_cl(x.float(), (224, 224))
            plan = ops.trunk_plan([(m.weight, m.bias, relu, pool) for m, relu, pool in layers], x.shape, x,
                                   arith=self.feature_arith)
            feats = ops.conv_trunk_forward(plan, x)                    # [N,h,w,C]: the NMF's layout already
            h, w, c = feats.shape[1:]
            return feats.view(b, nv * h * w, c), h, w
        x = F.interpolate(x, size=(224, 224), mode='bilinear', align_corners=False)
        features = self.net.features(x)
        c, h, w = features.shape[1:]
        return features.permute(0, 2, 3, 1).reshape(b, nv * h * w, c).float().contiguous(), h, w

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
            flat, h, w = self._features(imgs)
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
