"""The NumPy restatement of the partition distances (partdist_ref.py) against independent formulas, the host-only selection
credibleball_from_distances against the restated definition, and the conditions the GPU tests' inputs have to meet — all
without a GPU.  LOSS_TOL is test_gpu_visearch's: the table's rounding contributes at most 2·2^-32 ≈ 4.7e-10 to a VI (half of
that to an ID), the f64 sums of the plain formulas far less."""
import os

import numpy as np
import pytest

import partdist_ref as PD
import psm_search_ref as R
import vi_search_ref as V
import redclust_amd as rc
from redclust_amd import _lib
from test_gpu_visearch import LOSS_TOL, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in SHAPES if s[0] <= 65]
VARIED = [(65, 50, 5, 0.2), (257, 17, 16, 0.2)]
LOSSES = ("binder", "VI", "ID")


def planted(shape):
    n, m, K, noise = shape
    return R.planted_counts(n, m, K, noise, seed=1000 + n)[0]


def labellings_of(S):
    n = S.shape[1]
    rng = np.random.default_rng(n)
    return np.stack([np.ones(n, np.int64), np.arange(1, n + 1), S[0], rng.integers(1, 4, n), n + 1 - S[-1]])


def phi(x):
    x = x[x > 0].astype(np.float64)
    return float(np.sum(x * np.log(x)))


@pytest.mark.parametrize("shape", SMALL, ids=[f"n{s[0]}" for s in SMALL])
def test_binder_numerator_is_the_number_of_disagreeing_pairs(shape):
    S = planted(shape)
    labs = labellings_of(S)
    P, T, A, B = PD.distances_ref(labs, S, V.numpy_G(shape[0]))
    num = PD.numerators(P, T, A, B, "binder")
    iu = np.triu_indices(shape[0], 1)
    for l, c in enumerate(labs):
        for s, z in enumerate(S):
            same_c, same_z = (c[:, None] == c[None, :])[iu], (z[:, None] == z[None, :])[iu]
            assert num[l, s] == int((same_c != same_z).sum()), (l, s)


@pytest.mark.parametrize("shape", SHAPES[:6], ids=[f"n{s[0]}" for s in SHAPES[:6]])
def test_vi_and_id_numerators_against_the_search_criterion_and_the_plain_formulas(shape):
    n = shape[0]
    S = planted(shape)
    labs = labellings_of(S)
    G = V.numpy_G(n)
    P, T, A, B = PD.distances_ref(labs, S, G)
    vi, idn = PD.numerators(P, T, A, B, "VI"), PD.numerators(P, T, A, B, "ID")
    for l, c in enumerate(labs):
        assert sum(int(x) for x in vi[l]) == V.q_direct(c, S, G) + V.constant(S, G)
        cd = np.unique(c, return_inverse=True)[1]
        for s, z in enumerate(S):
            zd = np.unique(z, return_inverse=True)[1]
            a, b, t = phi(np.bincount(cd)), phi(np.bincount(zd)), phi(np.bincount(cd * (int(zd.max()) + 1) + zd))
            assert abs(int(vi[l, s]) / (2 ** 32 * n) - (a + b - 2 * t) / n) <= LOSS_TOL
            assert abs(int(idn[l, s]) / (2 ** 32 * n) - (max(a, b) - t) / n) <= LOSS_TOL


@pytest.mark.parametrize("shape", SHAPES[:6], ids=[f"n{s[0]}" for s in SHAPES[:6]])
def test_a_sample_is_at_distance_zero_from_itself(shape):
    S = planted(shape)
    P, T, A, B = PD.distances_ref(S, S, V.numpy_G(shape[0]))
    assert np.array_equal(A, B)
    assert np.array_equal(np.diag(P), B[:, 0]) and np.array_equal(np.diag(T), B[:, 1])
    for loss in LOSSES:
        num = PD.numerators(P, T, A, B, loss)
        assert not np.diag(num).any() and (num >= 0).all() and np.array_equal(num, num.T)


def test_credibleball_from_distances_on_a_case_worked_by_hand():
    num, K = [0, 3, 3, 5, 7, 9], [3, 2, 4, 2, 4, 5]
    # alpha = 0.34: k = 6 − ⌊2.04⌋ = 4, ε = 5, ball {0, 1, 2, 3}; fewest clusters 2: samples 1, 3, the farthest is 3; most 4: sample 2
    got = rc.credibleball_from_distances(num, K, 0.34)
    assert got["epsilon_num"] == 5 and got["level"] == 4 / 6 and got["ball"].tolist() == [True] * 4 + [False] * 2
    assert got["horizontal_index"].tolist() == [3] and got["upper_index"].tolist() == [3] and got["lower_index"].tolist() == [2]
    # alpha = 0.5: k = 3, ε = 3 with two samples there; alpha = 2/3: k = 2, the same radius, so the ball holds 3 > k samples
    for alpha in (0.5, 2 / 3):
        got = rc.credibleball_from_distances(num, K, alpha)
        assert got["epsilon_num"] == 3 and got["level"] == 0.5 and got["ball"].tolist() == [True] * 3 + [False] * 3
        assert got["horizontal_index"].tolist() == [1, 2] and got["upper_index"].tolist() == [1] and got["lower_index"].tolist() == [2]
    # alpha = 0: everything; the bounds are the farthest of the samples with 2 and with 5 clusters
    got = rc.credibleball_from_distances(num, K, 0.0)
    assert got["epsilon_num"] == 9 and got["level"] == 1.0 and got["ball"].all()
    assert got["horizontal_index"].tolist() == [5] and got["upper_index"].tolist() == [3] and got["lower_index"].tolist() == [5]
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            rc.credibleball_from_distances(num, K, bad)


def assert_ball_equal(got, ref):
    assert got["epsilon_num"] == ref["epsilon_num"] and got["level"] == ref["level"]
    assert np.array_equal(got["ball"], ref["ball"])
    for k in ("horizontal_index", "upper_index", "lower_index"):
        assert list(got[k]) == list(ref[k]), k


@pytest.mark.parametrize("seed", range(8))
def test_credibleball_from_distances_equals_the_restated_definition(seed):
    rng = np.random.default_rng(seed)
    m = int(rng.integers(1, 60))
    num, K = rng.integers(0, 12, m), rng.integers(1, 5, m)              # few values: ties everywhere
    for alpha in (0.0, 0.05, 0.25, 0.5, 0.99):
        assert_ball_equal(rc.credibleball_from_distances(num, K, alpha), PD.credibleball_ref(num, K, alpha))


def varied_balls(shape):
    n = shape[0]
    S = PD.varied_samples(*shape, seed=1000 + n)
    P, T, A, B = PD.distances_ref(S[:1], S, V.numpy_G(n))
    return S, {loss: PD.numerators(P, T, A, B, loss)[0] for loss in LOSSES}, B[:, 2]


def test_input_conditions_planted_samples_share_one_K_so_their_bounds_coincide():
    for shape in VARIED:
        S = planted(shape)
        assert len({len(np.unique(s)) for s in S}) == 1
        P, T, A, B = PD.distances_ref(S[:1], S, V.numpy_G(shape[0]))
        ref = PD.credibleball_ref(PD.numerators(P, T, A, B, "VI")[0], B[:, 2], 0.25)
        assert ref["horizontal_index"] == ref["upper_index"] == ref["lower_index"]


def test_input_conditions_varied_samples_separate_the_bounds():
    for shape in VARIED:
        S, nums, K = varied_balls(shape)
        assert len(set(K.tolist())) >= 3
        for loss in LOSSES:
            for alpha in (0.05, 0.25):
                ref = PD.credibleball_ref(nums[loss], K, alpha)
                assert ref["upper_index"] != ref["lower_index"], (shape, loss, alpha)
                if shape[0] == 257 and alpha == 0.25 and loss != "binder":
                    assert len({tuple(ref[k]) for k in ("horizontal_index", "upper_index", "lower_index")}) == 3, (shape, loss)


def test_input_conditions_a_tie_at_the_radius_makes_the_ball_larger_than_k():
    S = R.planted_counts(64, 7, 4, 0.1, seed=1064)[0]
    P, T, A, B = PD.distances_ref(S[:1], S, V.numpy_G(64))
    ref = PD.credibleball_ref(PD.numerators(P, T, A, B, "binder")[0], B[:, 2], 0.25)
    assert 7 - int(np.floor(0.25 * 7 + 1e-9)) == 6
    assert int(ref["ball"].sum()) == 7 and len(ref["horizontal_index"]) == 2


def test_arguments_are_checked_before_the_library_is_needed():
    S = planted(SHAPES[3])
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.partitiondistances(S[0], S, "omARI")
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.expecteddistances(S[0], S, "vi")
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.credibleball(S[0], S, "omARI")
    for bad in (-0.01, 1.0):
        with pytest.raises(ValueError):
            rc.credibleball(S[0], S, "VI", alpha=bad)
    with pytest.raises(ValueError):
        rc.partitiondistances(S[0][:-1], S)
    C = R.planted_counts(64, 7, 4, 0.1, seed=1064)[1]
    with pytest.raises(ValueError, match="exact=True needs the samples"):
        rc.hclustpointestimate(C, "VI", numsamples=7, exact=True)
    with pytest.raises(ValueError, match="exact=True needs the samples"):
        rc.hclustpointestimate(None, "VI", numsamples=7, ctx=object(), exact=True)
    with pytest.raises(ValueError, match="Invalid loss function specifier."):
        rc.hclustpointestimate(C, "ID", numsamples=7)                    # "ID" only together with exact=True


def test_the_entry_point_is_declared_bound_and_called_from_the_julia_glue():
    import test_oracle_cpu as T
    assert "rc_partition_distances" in _lib.SIGNATURES and len(_lib.SIGNATURES["rc_partition_distances"][1]) == 11
    hdr = open(os.path.join(ROOT, "include", "redclust_hip.h")).read()
    assert T._header_prototypes(hdr)["rc_partition_distances"] == (
        "int32_t", ["int32_t", "int64_t*", "int64_t", "int64_t", "int64_t", "int64_t*", "int64_t*", "int64_t*", "int64_t*", "int64_t*",
                    "double*"])
    jl = open(os.path.join(ROOT, "julia", "RedClustHIP.jl")).read()
    assert [c[0] for c in T._julia_ccalls(jl)].count("rc_partition_distances") >= 1
    assert "export partitiondistances, credibleball" in jl
    T.test_julia_glue_ccalls_match_the_header()
