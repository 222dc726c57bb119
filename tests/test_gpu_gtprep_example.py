"""GPU: the end-to-end example with the pansharpening loss (examples/train_synthetic.py --pansharp-loss brovey) at its
smallest size: the loss is finite and falls, and the recorded step (--graph) gives the eager run's bits."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_example_with_pansharp_loss_eager_and_graph():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    args = ["--gaussians", "2000", "--size", "64", "--iters", "12", "--quiet", "--no-prune", "--pansharp-loss", "brovey"]
    eager = train_synthetic.main(args)
    pansharp_first, pansharp_last = train_synthetic.main.last_pansharp_loss
    assert math.isfinite(eager[0]) and math.isfinite(eager[1]) and eager[1] < eager[0], eager
    assert math.isfinite(pansharp_last) and 0 < pansharp_last < pansharp_first  # the term itself is there and falls
    graph = train_synthetic.main(args + ["--graph"])
    assert graph == eager, (eager, graph)  # the same bits
    assert train_synthetic.main.last_pansharp_loss == (pansharp_first, pansharp_last)
    plain = train_synthetic.main(args[:-2])
    assert plain[0] != eager[0]  # the term is part of the loss
