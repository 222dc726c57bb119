"""GPU (MI355X): examples/train_synthetic.py --flow-matching --flow-network large --flow-update fused_large --flow-encoder
fused_large runs to the end, at the size tests/test_gpu_flownet_example.py uses, with finite losses."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_example_with_the_fused_large_encoders():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic

    first, last = train_synthetic.main(["--gaussians", "5000", "--size", "128", "--iters", "6", "--quiet", "--flow-matching",
                                        "--flow-network", "large", "--flow-update", "fused_large", "--flow-encoder", "fused_large"])[:2]
    assert math.isfinite(first) and math.isfinite(last)
    with pytest.raises(SystemExit):
        train_synthetic.main(["--gaussians", "5000", "--size", "128", "--iters", "1", "--quiet", "--flow-matching", "--flow-network", "small",
                              "--flow-encoder", "fused_large"])
