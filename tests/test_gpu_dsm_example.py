"""GPU: examples/train_synthetic.py --dsm-mae-every scores the altitude channel of the view's render as a DSM against the
altitude render of the unperturbed scene (eogs2_amd.dsm_eval.dsm_mae) while it trains."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_example_reports_the_dsm_mae():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    args = ["--gaussians", "20000", "--size", "160", "--iters", "30", "--quiet"]
    plain = train_synthetic.main(args)
    assert train_synthetic.main.last_dsm_mae == []  # off by default
    scored = train_synthetic.main(args + ["--dsm-mae-every", "10"])
    assert scored == plain  # scoring reads the render, it changes nothing
    scores = train_synthetic.main.last_dsm_mae
    assert [s[0] for s in scores] == [10, 20, 30]
    for it, dx, dy, mae in scores:
        assert isinstance(dx, int) and isinstance(dy, int) and abs(dx) <= 15 and abs(dy) <= 15
        assert math.isfinite(mae) and mae >= 0.0
    # as a replayed graph the kept altitude is the recorded step's output tensor, refilled by every replay: same scores
    graphed = train_synthetic.main(args + ["--dsm-mae-every", "10", "--graph"])
    assert graphed == plain and train_synthetic.main.last_dsm_mae == scores
    # whether the MAE falls is reported, not asserted: no measurement of it exists yet
    print("DSM MAE over the run (iteration, dx, dy, mae):", scores)
