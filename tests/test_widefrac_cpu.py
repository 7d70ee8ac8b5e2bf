"""csrc/widefrac.inc.hpp — the PEAR search's exact fraction where num and den pass 64 bits — on the host: tests/widefrac_host.cpp
reads lines "T m P X1 A1 X2 A2" and prints num and den of both candidates as (hi, lo) limbs and the verdict of the comparison;
every line is held to Python integers and fractions.Fraction.  The cases sit at the capacity of rc_pear_search_large
(n = 32767, m·n < 2^31), where num and den reach 74 bits and their cross products 148."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_hostmodel_cpu import SANITIZE

HERE = os.path.dirname(os.path.abspath(__file__))
N = 32767
T = N * (N - 1) // 2                       # 536 821 761, odd
M = (2 ** 31 - 1) // N                     # 65 538: the largest m with m·n < 2^31
ODD_M = 65537
C_SMALL = 1001                             # T·m − 2·P of the "lowest limb" cases
P_HALF = (T * ODD_M - C_SMALL) // 2


def near_half(A1, dv):
    """Two candidates at (T, ODD_M, P_HALF) with ΔA = 2, ΔX = m and 2·X1 − m·A1 = P + dv: then T·ΔX − P·ΔA = c and
    X1·A2 − X2·A1 = P + dv, so the cross products differ by 2·T·(c·(P + dv) − P·c) = 2·T·c·dv — about 2^40 per unit of dv,
    below one limb, on products of about 2^146; dv = 0 gives equal fractions with different (X, A)"""
    A1 += (ODD_M * A1 + dv + P_HALF) & 1                    # m is odd: the next A1 makes 2·X1 an even number
    X1 = (ODD_M * A1 + dv + P_HALF) // 2
    assert 2 * X1 - ODD_M * A1 == dv + P_HALF and X1 + ODD_M <= ODD_M * T
    return (T, ODD_M, P_HALF, X1, A1, X1 + ODD_M, A1 + 2)


def drawn(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        t, m = int(rng.integers(1, T + 1)), int(rng.integers(1, M + 1))
        out.append((t, m, int(rng.integers(0, m * t + 1))) + tuple(int(rng.integers(0, hi + 1)) for hi in (m * t, t, m * t, t)))
    return out


CASES = {
    "bounds": [(T, M, M * T, M * T, T, 0, 0), (T, M, M * T, 0, 0, M * T, 0), (T, M, 0, M * T, T, 0, T), (T, M, M * T // 2, M * T, T, 0, T),
               (T, M, M * T // 2, M * T, 1, M * T, T - 1), (T, M, 1, M * T, T - 1, M * T - 1, T), (T, 1, T, T, T, 1, 1),
               (T, M, M * T - 1, M * T, T, M * T, T - 1), (1, 1, 1, 1, 1, 0, 0), (1, M, M, 0, 1, M, 1)],
    "den_zero": [(0, 1, 0, 0, 0, 0, 0), (T, M, 0, 0, 0, 5, 3), (T, M, M * T, M * T, T, 7, 2), (T, M, M * T, 3, T, 4, T),
                 (T, M, 0, 0, 0, 0, 0), (6, 3, 0, 0, 0, 0, 6)],
    "negative": [(T, M, M * T // 3, 0, T // 2, 0, T // 3), (T, M, M * T // 3, 5, T, 6, T), (T, M, M * T - 1, 0, T - 1, 1, T - 1),
                 (T, M, M * T // 2, 0, T, M * T, T), (T, M, 12345, 0, 1, 0, 2), (T, ODD_M, P_HALF, 0, T - 1, 0, T)],
    "equal": [near_half(3 * T // 4, 0), near_half(T // 2 + 10, 0), near_half(T - 4, 0),
              (T, 6, 2 * T, 2 * 10, 10, 2 * 999, 999), (T, M, 3 * T, 3 * T, T, 0, 0), (T, 4, 2 * T, 100, 7, 100 + 2 * 5, 12)],
    "lowest_limb": [near_half(3 * T // 4, dv) for dv in (1, -1, 2, -2, 1000, -1000)] +
                   [near_half(T - 5, dv) for dv in (1, -1)],
    "drawn": drawn(200, 20261126),
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("widefrac") / "widefrac_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", path, os.path.join(HERE, "widefrac_host.cpp")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        print("built without the sanitizers")
        subprocess.check_call(cmd)
    return path


def exact(t, m, P, X, A):
    den = t * (m * A + P) - 2 * A * P
    assert den >= 0
    return (2 * (t * X - A * P), den) if den else (0, 1)


@pytest.mark.parametrize("group", list(CASES))
def test_fractions_and_verdicts_equal_python_integers(exe, group):
    lines = CASES[group]
    out = subprocess.run([exe], input="".join(" ".join(map(str, c)) + "\n" for c in lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [list(map(int, r.split())) for r in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    verdicts = set()
    for (t, m, P, X1, A1, X2, A2), row in zip(lines, rows):
        f = [exact(t, m, P, X1, A1), exact(t, m, P, X2, A2)]
        want = [w for num, den in f for v in (num, den) for w in (v >> 64, v & (2 ** 64 - 1))]
        a, b = Fraction(*f[0]), Fraction(*f[1])
        assert row == want + [(a > b) - (a < b)], (group, t, m, P, X1, A1, X2, A2)
        verdicts.add(row[-1])
        cross = (f[0][0] * f[1][1], f[1][0] * f[0][1])
        if group == "den_zero":
            assert (0, 1) in f
        if group == "negative":
            assert min(f[0][0], f[1][0]) < 0
        if group == "equal":
            assert a == b and (X1, A1) != (X2, A2)
        if group == "lowest_limb":
            assert min(map(abs, cross)) > 2 ** 128 and 0 < abs(cross[0] - cross[1]) < 2 ** 64
    if group in ("drawn", "lowest_limb"):
        assert verdicts >= {-1, 1}
