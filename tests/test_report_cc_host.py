"""CPU: the recomposition's own text (eogs2_amd/csrc/report_cc.h, what the kernel of csrc/report.hip compiles) on the host:
tests/report_cc_host.cpp, a program with its own main, built with the host compiler under AddressSanitizer and UBSan (nothing
preloaded) and -ffp-contract=off; with a compiler that lacks the sanitizers' runtimes it is built plain, and the suite's output
says which. On every fixture camera the results are numpy's float64 Ai inv(A1) and bi - Ai inv(A1) b1 rounded once: within
one fp32 ulp; the reference camera's own result is the identity and a zero bias to within one rounding; a singular A1 gives NaN."""
import numpy as np
import pytest

import report_cases as RC


@pytest.fixture(scope="module")
def recomposed():
    cases = []
    for case in RC.align_cases():
        z = RC.load_fixture(f"align_{case['name']}")
        ref = int(z["ref"])
        for v in range(z["weights"].shape[0]):
            cases.append((case["name"], v, ref, z["weights"][v], z["biases"][v], z["weights"][ref], z["biases"][ref]))
    return cases, RC.host_recompose([c[3:] for c in cases])


def test_host_program_build_is_reported(recomposed, capsys):
    """Whether the program ran under the sanitizers or, on a compiler without their runtimes, plain: said, not assumed."""
    built = RC.host_build()
    with capsys.disabled():
        print(f"\n  report_cc_host built {built}", end="")
    assert built in ("sanitized", "plain")


def test_float64_rounded_once_on_every_fixture_camera(recomposed):
    cases, outs = recomposed
    assert len(cases) == 9 * RC.N_CAMERAS
    for (name, v, ref, Ai, bi, A1, b1), (oA, ob) in zip(cases, outs):
        R, rb, magA, magb = RC.recompose_float64(Ai, bi, A1, b1)
        # (F64_NOISE: numpy's LU inverse and the closed form differ by float64 roundings at the size of the terms, which is all
        # that is left where a result cancels to nearly 0 — the reference camera's own off-diagonals)
        assert np.all(np.abs(oA.astype(np.float64) - R) <= RC.ulp32(R) + RC.F64_NOISE * magA), (name, v, oA, R)
        assert np.all(np.abs(ob.astype(np.float64) - rb) <= RC.ulp32(rb) + RC.F64_NOISE * magb), (name, v, ob, rb)


def test_reference_camera_becomes_the_identity(recomposed):
    cases, outs = recomposed
    seen = 0
    for (name, v, ref, Ai, bi, A1, b1), (oA, ob) in zip(cases, outs):
        if v != ref:
            continue
        seen += 1
        # one rounding: of 1 on the diagonal, of a float64 residue elsewhere
        _, _, magA, magb = RC.recompose_float64(Ai, bi, A1, b1)
        assert np.all(np.abs(oA.astype(np.float64) - np.eye(3)) <= RC.U * magA), (name, oA)
        assert np.all(np.abs(ob.astype(np.float64)) <= RC.U * magb), (name, ob)
    assert seen == 9


def test_singular_reference_gives_nan():
    Ai, bi, b1 = np.eye(3, dtype=np.float32), np.ones(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    outs = RC.host_recompose([(Ai, bi, A1, b1) for _, A1 in RC.SINGULAR])
    for (name, _), (oA, ob) in zip(RC.SINGULAR, outs):
        assert np.isnan(oA).all() and np.isnan(ob).all(), name
