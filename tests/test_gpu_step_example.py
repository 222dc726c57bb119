"""GPU: the end-to-end example with both optimizers inside the recorded step (examples/train_synthetic.py
--optimizer-in-graph: FusedAdam(capturable=True) behind eogs2_amd.rasterizer.captured_gate): the replayed graph gives the
run of the same optimizers stepped eagerly, bit for bit, with and without the retire inside the Adam launch."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--gaussians", "20000", "--size", "128", "--iters", "40", "--quiet", "--optimizer-in-graph"]


def _main():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    return train_synthetic.main


def test_optimizers_inside_the_graph_match_the_eager_run():
    main = _main()
    eager = main(ARGS)
    graph = main(ARGS + ["--graph"])
    assert graph == eager, (eager, graph)  # same losses, same Gaussians, bit for bit
    assert eager[1] < eager[0], eager


def test_retire_inside_the_adam_launch_with_deferred_compaction():
    main = _main()
    args = ARGS + ["--defer-prune", "3", "--prune-every", "10"]
    eager = main(args)
    graph = main(args + ["--graph"])
    assert graph == eager, (eager, graph)
    assert eager[1] < eager[0] and 0 < eager[2] <= 20000, eager
