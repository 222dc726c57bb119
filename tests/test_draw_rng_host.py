"""CPU: the generator's own text (eogs2_amd/csrc/draw_rng.h, what the kernel of csrc/draw.hip compiles) on the host:
tests/draw_rng_host.cpp, a program with its own main, built with the host compiler under AddressSanitizer and UBSan
(-fno-sanitize-recover=all, nothing preloaded). It checks the Random123 known-answer vectors of philox4x32-10, the counter's
layout, uniforms in [0, 1), u1 > 0, |z| <= 1, and over 65 536 consecutive iterations of one seed the share of normals at
+-1 (0.3173 +- 0.0091) and of positive normals (0.5 +- 0.0098)."""
import re

import draw_cases as DC


def test_host_program_passes_every_check():
    out, _ = DC.host_program()
    assert "ALL CHECKS PASSED" in out and "FAILED" not in out, out[-3000:]


def test_statistics_are_the_clipped_normals():
    out, _ = DC.host_program()
    stats = re.findall(r"STAT seed (\d+) component (\d) clipped ([0-9.]+) positive ([0-9.]+)", out)
    assert [c for _, c, _, _ in stats] == ["0", "1"]
    for _, _, clipped, positive in stats:
        assert abs(float(clipped) - 0.3173) <= 0.0091  # 5 sigma, sigma = sqrt(p (1 - p) / 65536)
        assert abs(float(positive) - 0.5) <= 0.0098


def test_sample_covers_the_carry_and_both_seed_ends():
    rows = DC.host_samples()
    assert len(rows) == 4 * 6 * 3
    assert {r[1] for r in rows} >= {0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1}
    assert {r[0] for r in rows} >= {0, 2 ** 64 - 1}
    assert len({tuple(r[3]) for r in rows}) == len(rows)  # every (seed, iteration, slot) has a block of its own
    first = next(r for r in rows if r[:3] == (0, 0, 0))
    assert tuple(first[3]) == DC.KAT[0][2]
    assert first[4] == [DC.f32_bits((w >> 8) * 2.0 ** -24) for w in DC.KAT[0][2][:3]]
