"""Child process of tests/test_gpu_adam.py::test_graph_capture_replays_the_step: optim.FlatAdam.step() captured into a graph.

Model A takes four eager steps (table path).  Model B takes the first step eagerly, then one step() is captured on the capture
stream -- under capture it packs the .grad tensors (bucket.gather(): one multi-tensor copy) and runs the flat kernel, two nodes in
a chain -- and is replayed three times with the .grad tensors refilled in place.  Both end with the same bits and counter 4."""
import os
import sys

import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
for d in (os.path.dirname(TESTS), TESTS):
    if d not in sys.path:
        sys.path.insert(0, d)


def main():
    import mvs_amd  # noqa: F401
    import adam_cases as AC
    from mvs_amd import _lib
    from mvs_amd.optim import FlatAdam
    dev = torch.device("cuda:0")
    lib = _lib.get()
    net_a, net_b = AC.small_model().to(dev), AC.small_model().to(dev)
    pa, pb = list(net_a.parameters()), list(net_b.parameters())
    grads = AC.model_grads(pa, 4)
    opt_a = FlatAdam(net_a.parameters(), lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=1e-2)
    opt_b = FlatAdam(net_b.parameters(), lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=1e-2)
    for gs in grads:
        opt_a.zero_grad()
        AC.assign_grads(pa, gs)
        opt_a.step()
    AC.assign_grads(pb, grads[0])                  # these .grad tensors stay: the graph reads them
    opt_b.step()
    torch.cuda.synchronize()
    lib.launch_trace()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_b.step()
    assert lib.launch_trace() == ["adam_flat"], "under capture the step takes the flat path"
    torch.cuda.synchronize()
    assert opt_b.steps_taken() == 1, "capturing must not run the step"
    for gs in grads[1:]:
        with torch.no_grad():
            for p, g in zip(pb, gs):
                p.grad.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert opt_b.steps_taken() == 4 and opt_a.steps_taken() == 4 and opt_b.counter.tolist() == [4, 0]
    AC.assert_bits_equal((opt_a.bucket.flat_param.data, opt_a.exp_avg, opt_a.exp_avg_sq),
                         (opt_b.bucket.flat_param.data, opt_b.exp_avg, opt_b.exp_avg_sq), "graph replay against eager steps")
    print("capture ok")


if __name__ == "__main__":
    main()
