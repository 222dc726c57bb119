"""GPU: the end-to-end example over several views (examples/train_synthetic.py --views V: eogs2_amd.views.ViewBank inside the
iteration). The recorded step with both optimizers, the bank's store and the cursor inside it gives the eager loop's run bit for
bit: losses, model parameters and every row of the bank; and one view stays what it was."""
import os
import sys

import pytest
import torch

import views_cases as VC

pytestmark = pytest.mark.gpu

ARGS = ["--gaussians", "20000", "--size", "128", "--iters", "12", "--quiet", "--optimizer-in-graph"]


def _example():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    return train_synthetic


def test_three_views_in_the_recorded_step_match_the_eager_loop():
    ex = _example()
    runs = []
    for extra in ([], ["--graph"]):
        out = ex.main(ARGS + ["--views", "3"] + extra)
        bank = ex.main.view_bank
        runs.append((out, ex.main.last_params, bank.state_dict(), bank.schedule.position(), bank.schedule.order.cpu().tolist()))
    (eager, e_params, e_rows, e_pos, order), (graph, g_params, g_rows, g_pos, g_order) = runs
    assert graph == eager, (eager, graph)  # same losses, same Gaussians
    assert e_pos == g_pos == 12 and order == g_order and sorted(set(order)) == [0, 1, 2]
    assert ex.main.last_step is not None and ex.main.last_step.replays >= 11  # (the graph run did replay)
    for k in e_params:
        assert VC.same_bits(e_params[k], g_params[k]), k
    assert sorted(e_rows) == sorted(g_rows) and len(e_rows) == 6 + 4 * 3
    for k in e_rows:
        assert VC.same_bits(e_rows[k], g_rows[k]), k
    # every camera moved on its own count: the steps are the visit counts, and the three cameras ended apart
    steps = [float(x) for x in e_rows["camera.0.step"]]
    assert steps == [float(c) for c in VC.visits(order, 3)] and sum(steps) == 12
    assert not VC.same_bits(e_rows["camera.0"][0], e_rows["camera.0"][1])
    assert eager[0] == eager[0] and eager[1] == eager[1]  # finite losses


def test_one_view_is_the_example_without_the_flag():
    ex = _example()
    args = ["--gaussians", "20000", "--size", "128", "--iters", "12", "--quiet"]
    plain = ex.main(args)
    assert ex.main.view_bank is None
    one = ex.main(args + ["--views", "1"])
    assert one == plain and ex.main.view_bank is None
