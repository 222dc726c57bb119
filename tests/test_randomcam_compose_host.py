"""CPU: the composition's own text (eogs2_amd/csrc/randomcam_compose.h, what the kernel of csrc/randomcam.hip compiles) on the
host: tests/randomcam_compose_host.cpp, a program with its own main, built with the host compiler under AddressSanitizer and
UBSan (nothing preloaded) and -ffp-contract=off; with a compiler that lacks the sanitizers' runtimes it is built plain, and the
suite's output says which. Shears and general matrices come out within one fp32 ulp of numpy's float64
inv(C) @ S and inv(C) @ S @ C; the identity gives camera_to_sun back bit for bit; a singular matrix gives NaN."""
import numpy as np
import pytest

import randomcam_cases as RC


@pytest.fixture(scope="module")
def composed():
    cases = RC.compose_cases()
    return cases, RC.host_compose([(c, s) for _, c, s in cases])


def test_host_program_build_is_reported(composed, capsys):
    """Whether the program ran under the sanitizers or, on a compiler without their runtimes, plain: said, not assumed."""
    built = RC.host_build()
    with capsys.disabled():
        print(f"\n  randomcam_compose_host built {built}", end="")
    assert built in ("sanitized", "plain")


def test_within_one_ulp_of_numpy_float64(composed):
    cases, outs = composed
    assert len(cases) >= 15
    for (name, c, s), (V, K) in zip(cases, outs):
        V64, K64 = RC.compose_float64(c, s)
        assert np.all(np.abs(V.astype(np.float64) - V64) <= RC.ulp32(V64)), (name, V, V64)
        assert np.all(np.abs(K.astype(np.float64) - K64) <= RC.ulp32(K64)), (name, K, K64)


def test_shear_inverse_is_the_negated_shear(composed):
    cases, outs = composed
    for (name, c, s), (V, K) in zip(cases, outs):
        if name.startswith("shear"):
            exact = RC.shear(-c[0, 2], -c[1, 2]).astype(np.float64) @ s.astype(np.float64)  # rows 0, 1: s_ij - a s_2j
            assert np.all(np.abs(V.astype(np.float64) - exact) <= RC.ulp32(exact)), name
            assert np.array_equal(V[2], s[2]), name  # the last row passes untouched


def test_identity_returns_camera_to_sun_bit_for_bit(composed):
    cases, outs = composed
    name, c, s = cases[0]
    assert name == "identity"
    V, K = outs[0]
    assert V.tobytes() == s.tobytes() and K.tobytes() == s.tobytes()


def test_singular_gives_nan():
    s = RC.shear(0.25, -0.5)
    outs = RC.host_compose([(c, s) for _, c in RC.SINGULAR])
    for (name, _), (V, K) in zip(RC.SINGULAR, outs):
        assert np.isnan(V).all() and np.isnan(K).all(), name
