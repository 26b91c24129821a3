"""GPU: the fused Adam kernels and optim.FlatAdam on the MI355X -- the cases of tests/test_adam.py (tests/adam_cases.py) on the
device, and one step() captured into a graph and replayed."""
import os
import subprocess
import sys

import pytest
import torch

import adam_cases as AC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs cuda:0")]
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    from mvs_amd import _lib
    _lib._INSTANCE = None
    return torch.device("cuda:0")


def _flat_cases():
    cases = [(i, 0.0, 1.0) for i in range(8)]
    return cases + [(7, 1e-2, 1.0), (7, 0.0, 0.125), (7, 1e-2, 0.125), (6, 1e-2, 0.125)]


@pytest.mark.parametrize("size_index,wd,scale", _flat_cases())
def test_flat_accuracy(dev, size_index, wd, scale):
    AC.check_flat_accuracy(dev, AC.flat_sizes()[size_index], wd, scale)


@pytest.mark.parametrize("leads", [(1, 1, 1), (3, 3, 3), (0, 1, 2), (4, 4, 5)])
def test_flat_accuracy_at_other_alignments(dev, leads):
    AC.check_flat_accuracy(dev, AC.flat_sizes()[7], 1e-2, 0.125, leads=leads)


@pytest.mark.parametrize("kind", ["lengths", "null", "many", "many+1", "view"])
@pytest.mark.parametrize("leads,wd,scale", [((4, 4, 4), 0.0, 1.0), ((1, 1, 1), 1e-2, 0.125), ((0, 3, 2), 1e-2, 1.0)])
def test_table_path_equals_flat_path(dev, kind, leads, wd, scale):
    AC.check_table_equals_flat(dev, kind, leads=leads, wd=wd, grad_scale=scale)


def test_uncovered_elements_untouched(dev):
    AC.check_uncovered_elements_untouched(dev)


def test_exact_properties(dev):
    AC.check_exact_properties(dev)


def test_flat_adam_against_stock_adam_small_model(dev):
    AC.check_flat_adam_on_model(dev, AC.small_model(), "small model")


def test_flat_adam_against_stock_adam_mvsnet(dev):
    from mvs_amd.jdacs.models.mvsnet import MVSNet
    torch.manual_seed(0)
    AC.check_flat_adam_on_model(dev, MVSNet(refine=True), "MVSNet(refine=True)")


def test_graph_capture_replays_the_step():
    """One step() captured in a torch.cuda.graph on a single stream (flat path: gather + one kernel, no parallel branch), replayed three
    times with refilled gradients: bit-identical to four eager steps, counter 4.  In a child process under its own time limit
    (tests/adam_capture_child.py), so that a replay that hangs ends there."""
    r = subprocess.run([sys.executable, os.path.join(TESTS, "adam_capture_child.py")], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "capture ok" in r.stdout
