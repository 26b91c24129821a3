"""The optimiser both training scripts build -- optim.Adam(model.parameters(), lr, betas=(0.9, 0.999), weight_decay=wd)
(jdacs/train.py:71, jdacs-ms/train.py:101), stepped at train.py:208 / :260 -- as ONE HIP launch per step over the flat parameter
store of dist.FlatGradBucket(flatten_params=True) (csrc/adam_kernels.h; C ABI mvs_adam_step / mvs_adam_step_table).

    opt = mvs_amd.optim.FlatAdam(model.parameters(), lr=args.lr, betas=(0.9, 0.999), weight_decay=args.wd)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones, gamma)        # unchanged
    ...
    opt.zero_grad(); loss.backward(); opt.step()

Checkpoints are torch.optim.Adam's: ``state_dict()`` / ``load_state_dict()`` speak stock Adam's format over the model's own
parameters, so a checkpoint of the reference's train.py resumes here and one written here resumes there.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.distributed as dist

from . import _lib
from .dist import FlatGradBucket


class FlatAdam(torch.optim.Optimizer):
    """Adam (torch.optim.Adam's arithmetic: L2 weight decay, bias-corrected, no amsgrad) for parameters that live in one flat store.

    params: ``model.parameters()`` (or one parameter group as a dict).  Unless ``bucket`` is given, a
    ``FlatGradBucket(params, flatten_params=True)`` is built here -- the parameters become views of its flat store -- and is
    exposed as ``.bucket``.  Build the optimiser after every layout / dtype / device conversion of the model.

    ``step()`` is one launch.  Without a collective it reads the gradients where autograd left them (the parameters' ``.grad``
    tensors, through a table of pointers in the kernel's arguments): no gather, no copy.  When a collective is needed (world size
    above 1, or ``bucket.force_collective``), when the stream is being captured into a graph, or when a gradient is not an fp32
    tensor laid out with its parameter's strides, it packs the gradients (``bucket.gather()``), all-reduces the SUM and runs the
    flat kernel with the 1/world factor fused in.  Both paths give the same bits.

    ``lr`` (and every other hyper-parameter) is read from ``param_groups[0]`` at every call, so ``MultiStepLR`` works unchanged.
    UNDER GRAPH CAPTURE THE VALUE OF lr IS BAKED INTO THE GRAPH: re-capture after the schedule changes it.  The step count is not
    baked: it lives on the device and a replay advances it.

    ``exp_avg``, ``exp_avg_sq`` and the step counter live in ONE device buffer (``state_buffer``: floats [m | v | counter]), so
    restoring the optimiser to its initial state is one memset, and a snapshot is one copy.

    Two differences from stock Adam, both documented in INTEGRATION.md: the step counter is shared, so every parameter reports the
    same ``step``; and a parameter that received no gradient is updated with a gradient of zeros (``FlatGradBucket.gather()``'s
    meaning) where stock Adam skips it."""

    force_flat = False      # True: always pack the gradients and run the flat kernel (tools/adam_bench.py measures that path)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, amsgrad=False, maximize=False, bucket=None):
        if amsgrad or maximize:
            raise ValueError("FlatAdam: amsgrad / maximize are not served (torch.optim.Adam has them)")
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError("FlatAdam: exactly one parameter group is served, got %d" % len(params))
        # the param-group keys stock Adam writes in this torch version (amsgrad, maximize, foreach, capturable, ...), at its defaults
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("FlatAdam: amsgrad / maximize are not served (torch.optim.Adam has them)")
        self._check_hyper(group)
        trainable = [p for p in group["params"] if p.requires_grad]
        if bucket is None:
            bucket = FlatGradBucket(trainable, flatten_params=True)
        elif bucket.flat_param is None:
            raise ValueError("FlatAdam: the bucket must be a FlatGradBucket(flatten_params=True)")
        elif len(bucket.params) != len(trainable) or any(a is not b for a, b in zip(bucket.params, trainable)):
            raise ValueError("FlatAdam: the bucket's parameters must be the trainable ones of `params`, in the same order")
        self.bucket = bucket
        store = bucket.flat_param.data
        if store.dtype != torch.float32:
            raise TypeError("FlatAdam: fp32 parameters required, got %s" % store.dtype)
        n = store.numel()
        npad = n + (-n) % 4                                  # exp_avg_sq and the counter start 16-byte aligned like exp_avg
        self.state_buffer = torch.zeros(2 * npad + 4, dtype=torch.float32, device=store.device)
        self.exp_avg = self.state_buffer[:n]
        self.exp_avg_sq = self.state_buffer[npad:npad + n]
        self.counter = self.state_buffer[2 * npad:2 * npad + 2].view(torch.int32)     # [steps taken, scratch (0 between launches)]
        self._index = {id(p): i for i, p in enumerate(group["params"])}
        nseg = len(bucket.params)
        self._offsets, off = [], 0
        for p in bucket.params:
            self._offsets.append(off)
            off += p.numel()
        self._strides = [p.stride() for p in bucket.params]
        self._c_offs = (C.c_longlong * nseg)(*self._offsets)
        self._c_cnts = (C.c_longlong * nseg)(*[p.numel() for p in bucket.params])
        self._c_ptrs = (C.c_void_p * nseg)()
        self._param_ptrs = None

    @staticmethod
    def _check_hyper(g):
        if not 0.0 <= g["lr"]:
            raise ValueError("FlatAdam: invalid learning rate %r" % (g["lr"],))
        if not 0.0 <= g["eps"]:
            raise ValueError("FlatAdam: invalid epsilon %r" % (g["eps"],))
        if not (0.0 <= g["betas"][0] < 1.0 and 0.0 <= g["betas"][1] < 1.0):
            raise ValueError("FlatAdam: invalid betas %r" % (g["betas"],))
        if not 0.0 <= g["weight_decay"]:
            raise ValueError("FlatAdam: invalid weight_decay %r" % (g["weight_decay"],))

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("FlatAdam: exactly one parameter group is served")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Drops the parameters' .grad (as bucket.zero() does), so autograd WRITES fresh gradients instead of accumulating."""
        self.bucket.zero()

    # ---- the step ---------------------------------------------------------------------------------------------------------
    def _table_ready(self) -> bool:
        """Fills the pointer table from the parameters' .grad tensors; False when one of them cannot be read in place."""
        bucket = self.bucket
        store = bucket.flat_param.data
        ptrs = tuple(p.data_ptr() for p in bucket.params)
        if ptrs != self._param_ptrs:                          # a parameter was re-allocated: it must still alias the store, in place
            base = store.data_ptr()
            for p, ptr, off in zip(bucket.params, ptrs, self._offsets):
                if ptr != base + 4 * off:
                    raise RuntimeError("FlatAdam: a parameter of shape %s no longer aliases its range of the flat store; build the "
                                       "optimiser after every layout / dtype conversion of the model" % (tuple(p.shape),))
            self._strides = [p.stride() for p in bucket.params]
            self._param_ptrs = ptrs
        # a .grad is on its parameter's device and strided by torch's own rule for assigning one; dtype and strides are checked here
        f32, out = torch.float32, []
        for p, strides in zip(bucket.params, self._strides):
            g = p.grad
            if g is None:
                out.append(None)
            elif g.dtype is f32 and g.stride() == strides:
                out.append(g.data_ptr())
            else:
                return False
        self._c_ptrs[:] = out
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        bucket = self.bucket
        store = bucket.flat_param.data
        lib = _lib.get()
        if store.device.type != lib.device_type:
            raise RuntimeError("mvs_amd: parameters on %s but the HIP library serves '%s' devices; the optimiser step has no "
                               "CPU fallback" % (store.device, lib.device_type))
        stream = torch.cuda.current_stream(store.device).cuda_stream if store.is_cuda else None
        hyper = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
        collective = bucket.needs_collective()
        capturing = store.is_cuda and torch.cuda.is_current_stream_capturing()
        if not collective and not capturing and not self.force_flat and self._table_ready():
            lib.call("mvs_adam_step_table", store.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), store.numel(),
                     self._c_ptrs, self._c_offs, self._c_cnts, len(self._c_offs), self.counter.data_ptr(), *hyper, 1.0, stream)
            return loss
        bucket.gather()
        scale = 1.0
        if collective:
            bucket.all_reduce(average=False)                 # the sum; 1/world goes into the kernel
            scale = 1.0 / dist.get_world_size()
        lib.call("mvs_adam_step", store.data_ptr(), bucket.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                 store.numel(), self.counter.data_ptr(), *hyper, scale, stream)
        return loss

    # ---- checkpoints in torch.optim.Adam's format ---------------------------------------------------------------------------
    def steps_taken(self) -> int:
        """The device counter, read back (synchronises)."""
        return int(self.counter[0].item())

    def _state_views(self, p, k):
        off, n = self._offsets[k], p.numel()
        return (self.exp_avg[off:off + n].as_strided(p.shape, p.stride()), self.exp_avg_sq[off:off + n].as_strided(p.shape, p.stride()))

    def state_dict(self):
        """torch.optim.Adam's state_dict over the model's own parameters: per parameter ``step`` (the shared counter), ``exp_avg``
        and ``exp_avg_sq`` in the parameter's logical shape (a channels-last parameter's state is re-strided from storage order),
        and the param-group keys stock Adam writes.  Empty state before the first step, as stock Adam's."""
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self.param_groups[0]["params"])))
        state = {}
        t = self.steps_taken()
        if t > 0:
            for k, p in enumerate(self.bucket.params):
                m, v = self._state_views(p, k)
                state[self._index[id(p)]] = {"step": torch.tensor(float(t)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict):
        """Accepts what torch.optim.Adam.state_dict() (or this class's) wrote for the same model.  Parameters without an entry
        start from zero state; entries whose ``step`` values differ cannot be represented by the shared counter and raise."""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError("FlatAdam: the checkpoint has %d parameter groups, exactly one is served" % len(groups))
        mine = self.param_groups[0]
        if len(groups[0]["params"]) != len(mine["params"]):
            raise ValueError("FlatAdam: the checkpoint's group has %d parameters, this optimiser's %d"
                             % (len(groups[0]["params"]), len(mine["params"])))
        if groups[0].get("amsgrad") or groups[0].get("maximize"):
            raise ValueError("FlatAdam: the checkpoint was written with amsgrad / maximize, which are not served")
        pos = {saved: i for i, saved in enumerate(groups[0]["params"])}       # saved id -> position in the group
        entries = {}
        for saved, st in state_dict["state"].items():
            if saved not in pos:
                raise ValueError("FlatAdam: the checkpoint has state for parameter id %r, which is in no group" % (saved,))
            entries[pos[saved]] = st
        steps = {int(round(float(st["step"]))) for st in entries.values()}
        if len(steps) > 1:
            raise ValueError("FlatAdam: the checkpoint's parameters are at different steps %s; this optimiser keeps ONE step "
                             "counter for all of them" % sorted(steps))
        new_m, new_v = torch.zeros_like(self.exp_avg), torch.zeros_like(self.exp_avg_sq)
        for k, p in enumerate(self.bucket.params):
            st = entries.pop(self._index[id(p)], None)
            if st is None:
                continue
            off, n = self._offsets[k], p.numel()
            for buf, key in ((new_m, "exp_avg"), (new_v, "exp_avg_sq")):
                t = st[key]
                if tuple(t.shape) != tuple(p.shape):
                    raise ValueError("FlatAdam: %s of parameter %d has shape %s, the parameter %s"
                                     % (key, self._index[id(p)], tuple(t.shape), tuple(p.shape)))
                buf[off:off + n].as_strided(p.shape, p.stride()).copy_(t)
        if entries:
            raise ValueError("FlatAdam: the checkpoint has state for parameters %s, which do not require a gradient here" % sorted(entries))
        for key, val in groups[0].items():
            if key != "params":
                mine[key] = tuple(val) if key == "betas" else val
        self._check_hyper(mine)
        self.exp_avg.copy_(new_m)
        self.exp_avg_sq.copy_(new_v)
        self.counter.zero_()
        self.counter[0] = steps.pop() if steps else 0
