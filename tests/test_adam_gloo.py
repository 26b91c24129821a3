"""CPU, world size 2 over gloo, kernels on the emulation build: optim.FlatAdam's collective path -- gather, all-reduce of the SUM,
flat kernel with grad_scale = 1/world -- leaves both ranks with the parameters of a single-process step on the mean gradient."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _use_emulation():
    for d in (ROOT, TESTS):
        if d not in sys.path:
            sys.path.insert(0, d)
    import mvs_amd  # noqa: F401
    from mvs_amd import _lib
    import emul_util
    _lib._INSTANCE = _lib.MvsLib(emul_util.build_emul(), device_type="cpu")
    return _lib._INSTANCE


def _worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    lib = _use_emulation()
    import adam_cases as AC
    from mvs_amd import dist as mdist
    from mvs_amd.optim import FlatAdam
    mdist.init_from_env("gloo")
    net = AC.small_model(seed=100 + rank)                    # deliberately different per rank: the broadcast fixes it
    mdist.broadcast_parameters(net)
    params = list(net.parameters())
    ret["p0_%d" % rank] = [p.detach().clone() for p in params]
    opt = FlatAdam(net.parameters(), lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=1e-2)
    grads = AC.model_grads(params, 2, seed=rank)             # every rank its own gradients
    ret["grads_%d" % rank] = grads
    for gs in grads:
        opt.zero_grad()
        AC.assign_grads(params, gs)
        lib.launch_trace()
        opt.step()
        assert lib.launch_trace() == ["adam_flat"]
    ret["flat_%d" % rank] = opt.bucket.flat.clone()          # all_reduce(average=False): the SUM stays in the bucket
    ret["p_%d" % rank] = opt.bucket.flat_param.data.clone()
    ret["steps_%d" % rank] = opt.steps_taken()
    # the keyword's default is the behaviour from before: the mean
    opt.bucket.flat.copy_(torch.full_like(opt.bucket.flat, float(rank + 1)))
    opt.bucket.all_reduce()
    ret["mean_%d" % rank] = opt.bucket.flat.clone()
    opt.bucket.flat.copy_(torch.full_like(opt.bucket.flat, float(rank + 1)))
    opt.bucket.all_reduce(average=False)
    ret["sum_%d" % rank] = opt.bucket.flat.clone()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_step_on_the_mean_gradient():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    lib = _use_emulation()
    from mvs_amd import _lib
    import adam_cases as AC
    from mvs_amd.optim import FlatAdam
    try:
        assert ret["steps_0"] == ret["steps_1"] == 2
        assert torch.equal(ret["p_0"], ret["p_1"]), "the ranks ended with different parameters"
        assert all(torch.equal(a, b) for a, b in zip(ret["p0_0"], ret["p0_1"]))
        # one process, the mean gradient: (g0 + g1) * 0.5 is what the kernel forms from the summed bucket and grad_scale = 1/2
        net = AC.small_model()
        params = list(net.parameters())
        with torch.no_grad():
            for p, q in zip(params, ret["p0_0"]):
                p.copy_(q)
        opt = FlatAdam(net.parameters(), lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=1e-2)
        for g0, g1 in zip(ret["grads_0"], ret["grads_1"]):
            AC.assign_grads(params, [(a + b) * 0.5 for a, b in zip(g0, g1)])
            opt.step()
        assert torch.equal(opt.bucket.flat_param.data.view(torch.int32), ret["p_0"].view(torch.int32))
        # the bucket holds the sum of the last step's gradients, in storage order
        last = [a + b for a, b in zip(ret["grads_0"][-1], ret["grads_1"][-1])]
        want = torch.cat([torch.empty_strided(p.shape, p.stride()).copy_(g).as_strided((p.numel(),), (1,)) for p, g in zip(params, last)])
        assert torch.equal(ret["flat_0"], want) and torch.equal(ret["flat_1"], want)
        assert bool((ret["mean_0"] == 1.5).all()) and bool((ret["sum_0"] == 3.0).all()) and bool((ret["sum_1"] == 3.0).all())
    finally:
        _lib._INSTANCE = None
    assert lib is not None
