"""Distance matrices in other units (tests/test_units_cpu.py, tests/test_gpu_units.py) — TEST INFRASTRUCTURE.

One base matrix D0 per size (generatemixture, the points shuffled so that the labels are not contiguous and the layout code runs)
and named variants of it, each with its own likelihood hyperparameters:

  x2^-20, x2^20, x2^-60, x2^60   D0·2^s: the same mantissas, every fixed-point integer the same, the exponents shifted by -s
  x1e-6, x1e6                    D0·c, c no power of two: new mantissas
  below_one                      D0 / (2·max D0): every logarithm negative
  near_one                       the off-diagonal entries squeezed affinely into [0.94, 1.06]: the largest exponent of logD, entries
                                 in the two binades around 1.0
  near_one x2^-60, near_one x2^60
                                 that matrix ·2^∓60 (no longer near one: two binades at the far ends of the range)
  integers                       ceil(D0): a handful of distinct values, exact powers of two among them (zero mantissa)
  all_ones                       every off-diagonal entry 1.0: every logarithm 0

The hyperparameters are likelihood_hyperparams of the variant under the true labels.  all_ones has no such fit (the gamma shape
estimate needs log(mean) > mean(log)): it takes the base matrix's.
"""
import functools

import numpy as np

import redclust_amd as rc

SIZES = (333, 1029)            # inside one 1024 stride and no multiple of 64; just over the stride
K, SIGMA, DIM = 5, 0.3, 6
KCAP = 64                      # initial slot capacity of the contexts; tests/test_units_cpu.py keeps every chain's K below it
SEED = 20                      # of every sweep
NSWEEPS = 6
SM_SEED, SM_PROPOSALS = 11, 10   # the split–merge leg: proposals from sm_start, then a sweep

DYADIC = {"x2^-20": -20, "x2^20": 20, "x2^-60": -60, "x2^60": 60}
RESCALED = dict({k: 2.0 ** s for k, s in DYADIC.items()}, **{"x1e-6": 1e-6, "x1e6": 1e6})
# D0 spans five binades or more, so the log table with the exponent folded in (at most four) is reached by near_one, integers and
# all_ones only: near_one once more at 2^±60, for that table with eD > 100 and eD < 0
NEAR_ONE_DYADIC = {"near_one x2^-60": -60, "near_one x2^60": 60}
NAMES = ("base", "x2^-20", "x2^20", "x1e-6", "x1e6", "x2^-60", "x2^60", "below_one", "near_one", "integers", "all_ones",
         "near_one x2^-60", "near_one x2^60")
NEAR_ONE = (0.94, 1.06)


def dyadic_pair(name):
    """(the member this one is a power of two times, the power) or None"""
    if name in DYADIC:
        return "base", DYADIC[name]
    if name in NEAR_ONE_DYADIC:
        return "near_one", NEAR_ONE_DYADIC[name]
    return None


def rp(t):
    return 1.0 + 0.1 * t, 0.5


@functools.lru_cache(maxsize=None)
def base(n):
    """dict(points, D, truth, init): the shuffled data set and the perturbed start (every fifth label re-drawn)"""
    data = rc.generatemixture(n, K, seed=n, sigma=SIGMA, dim=DIM)
    sh = np.random.default_rng(n).permutation(n)
    D = np.ascontiguousarray(data["distancematrix"][np.ix_(sh, sh)])
    truth = np.ascontiguousarray(data["clusts"][sh])
    init = truth.copy()
    init[::5] = np.random.default_rng(1).integers(1, K + 1, len(init[::5]))
    out = dict(points=np.ascontiguousarray(data["points"][sh]), D=D, truth=truth, init=init)
    for v in out.values():
        v.setflags(write=False)
    return out


def sm_start(n):
    """the true labels with clusters 1 and 2 merged and clusters 3 and 4 each cut in two at random: proposals worth accepting"""
    z = base(n)["truth"].copy()
    z[z == 2] = 1
    rng = np.random.default_rng(3)
    for k, new in ((3, K + 1), (4, K + 2)):
        idx = np.flatnonzero(z == k)
        z[idx[rng.random(len(idx)) < 0.5]] = new
    return z


def scale_of(name):
    """the factor of a pure rescaling, None for the other members"""
    return 1.0 if name == "base" else RESCALED.get(name)


@functools.lru_cache(maxsize=None)
def member(name, n):
    """dict(name, D, P, truth, init, scale): D symmetric with a zero diagonal, P its likelihood hyperparameters"""
    b = base(n)
    D0 = b["D"]
    off = ~np.eye(n, dtype=bool)
    if scale_of(name) is not None:
        D = D0 * scale_of(name)
    elif name in NEAR_ONE_DYADIC:
        D = member("near_one", n)["D"] * 2.0 ** NEAR_ONE_DYADIC[name]
    elif name == "below_one":
        D = D0 / (2.0 * D0.max())
    elif name == "near_one":
        lo, hi = D0[off].min(), D0[off].max()
        D = NEAR_ONE[0] + (D0 - lo) * ((NEAR_ONE[1] - NEAR_ONE[0]) / (hi - lo))
        D = np.minimum(np.maximum(D, NEAR_ONE[0]), NEAR_ONE[1])       # (the affine map's own rounding at the two ends)
    elif name == "integers":
        D = np.ceil(D0)
    elif name == "all_ones":
        D = np.ones((n, n))
    else:
        raise KeyError(name)
    D = np.where(off, D, 0.0)
    assert np.array_equal(D, D.T)
    P = rc.likelihood_hyperparams(D0 if name == "all_ones" else D, b["truth"])
    D.setflags(write=False)
    return dict(name=name, D=D, P=P, truth=b["truth"], init=b["init"], scale=scale_of(name))


PREDICT_ROWS = ("training scale", "2^20 farther", "all ones", "near one", "x2^-60", "x1e6", "integers", "below one")


@functools.lru_cache(maxsize=None)
def predict_case(n=SIZES[0], m=6, sweeps=2):
    """Eight new points against the n training points of base(n), each row of distances in units of its own (PREDICT_ROWS),
    and six labellings of the training points: the truth, the perturbed start, one cluster, all singletons and two random ones.
    Dnn, for the joint call: the distances among the new points at the training scale, but those of "below one", "integers",
    "near one" and "all ones" in the units of their rows — the extended row of "all ones" still has no nonzero logarithm, that of
    "near one" still the largest exponent; "x2^-60" beside distances of order one quantises its training distances to zero."""
    b = base(n)
    rng = np.random.default_rng(77)
    q = len(PREDICT_ROWS)
    new = b["points"][rng.choice(n, q, replace=False)] + rng.normal(0.0, 0.05, (q, DIM))
    D0 = np.sqrt(((new[:, None, :] - b["points"][None, :, :]) ** 2).sum(axis=2))
    N0 = np.sqrt(((new[:, None, :] - new[None, :, :]) ** 2).sum(axis=2))
    off = b["D"][~np.eye(n, dtype=bool)]
    lo, hi = off.min(), off.max()
    Dnew = D0.copy()
    Dnew[1] *= 2.0 ** 20
    Dnew[2] = 1.0
    Dnew[3] = np.clip(NEAR_ONE[0] + (D0[3] - lo) * ((NEAR_ONE[1] - NEAR_ONE[0]) / (hi - lo)), *NEAR_ONE)
    Dnew[4] *= 2.0 ** -60
    Dnew[5] *= 1e6
    Dnew[6] = np.ceil(D0[6])
    Dnew[7] = D0[7] / (2.0 * hi)
    Dnn = N0.copy()                                  # (Dnn must be symmetric: a later line overrides an earlier one where two meet)
    for i, row in ((7, N0[7] / (2.0 * hi)), (6, np.ceil(N0[6])),
                   (3, np.clip(NEAR_ONE[0] + (N0[3] - lo) * ((NEAR_ONE[1] - NEAR_ONE[0]) / (hi - lo)), *NEAR_ONE)), (2, np.ones(q))):
        Dnn[i, :] = row; Dnn[:, i] = row
    np.fill_diagonal(Dnn, 0.0)
    S = np.stack([b["truth"], b["init"], np.full(n, n), rng.permutation(n) + 1,
                  (rng.choice(n, 7, replace=False) + 1)[rng.integers(0, 7, n)],
                  (rng.choice(n, 12, replace=False) + 1)[rng.integers(0, 12, n)]]).astype(np.int64)[:m]
    P = dict(member("base", n)["P"], maxK=0)
    Ln = np.log(np.where(np.eye(q, dtype=bool), 1.0, Dnn))
    return dict(Dnew=Dnew, logDnew=np.log(Dnew), Dnn=Dnn, logDnn=Ln, samples=S, r=rng.uniform(0.5, 3.0, len(S)),
                p=rng.uniform(0.1, 0.9, len(S)), P=P, seed=4077, sample_offset=0, point_offset=0, sweeps=sweeps)


def row_exponents(rows, logrows, count):
    """per-row (eD, eL) of rc_predict / rc_predict_joint: 62 - ex - ceil(log2 count) of the row's largest entry and of its largest
    |log|; 0 for a row of zeros"""
    e = lambda x: 62 - exponent(x) - ceil_log2(count) if x > 0 else 0
    return (np.array([e(float(np.abs(r).max())) for r in rows], np.int32),
            np.array([e(float(np.abs(r).max())) for r in logrows], np.int32))


def host_log(D):
    """log.(D - Diagonal(D) + I)"""
    return np.log(np.where(np.eye(D.shape[0], dtype=bool), 1.0, D))


def exponent(x):
    """ex of frexp: x < 2^ex"""
    return int(np.frexp(float(x))[1])


def ceil_log2(n):
    return int(n - 1).bit_length()


def expected_exponents(D, n, kind):
    """(eD, eL) of DESIGN.md §3 for a context of this kind ("derived", "stored", "bits32"; a context made from points is
    "derived") from the host's matrix: 62 - ex - ceil(log2 n) for 64-bit storage, 30 - ex for 32-bit, 0 for a matrix of zeros;
    a derived context caps eD at 47 - ex(max D) and eL at 50 - ex(max |log D|)."""
    L = host_log(D)
    mD, mL = float(D.max()), float(np.abs(L).max())
    if kind == "bits32":
        return 30 - exponent(mD), (30 - exponent(mL) if mL > 0 else 0)
    eD, eL = 62 - exponent(mD) - ceil_log2(n), (62 - exponent(mL) - ceil_log2(n) if mL > 0 else 0)
    if kind == "derived":
        eD = min(eD, 47 - exponent(mD))
        if mL > 0:
            eL = min(eL, 50 - exponent(mL))
    return eD, eL
