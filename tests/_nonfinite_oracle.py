"""Inputs whose scores leave the finite normal range -- NaN, +-inf, overflow, subnormals -- for the kernels that rank by score (K4, K6,
K8, K12), and the contract they are held to (include/tkr.h, K4): NaN > +inf > finite > -inf, every NaN the same score, -0.0 == +0.0,
ties -> higher column first; np.argsort(kind='stable') read backwards.

Every factor is a small integer times a power of two, so the finite part of every score is exact in any order of summation: ties are
exact, no entry has to be left out as a rounding hazard, and where an overflow makes the order matter the chain of
oracle/ref_np.mfma_chain_scores is the specification.  One remark on that chain: its steps are FUSED, the product is not rounded, so
finite factors never give a NaN (fma(2^100, -2^100, +inf) is +inf, not inf - inf) -- NaN scores need a NaN or an infinite factor.
Not a test module."""
import functools

import numpy as np

from oracle import ref_np as R

F32 = np.float32
WIDTHS = [50, 128, 300, 769]                 # bound-and-refine (two widths), the slab kernel, the wave-per-row kernels
N_ROWS, N_COLS, TOP = 130, 333, 30           # two user blocks of 128 with a tail; a tail tile
SPLIT = (700, 20000, 64)                     # rows, columns, k: the shape of test_item_range_split_is_invisible (item ranges share bounds)
# the cases run at the SPLIT shape: those whose factors are plain integers, for which split_scores below is exact without walking the
# chain over 14 M entries (the scaled cases -- overflow, huge_u, tiny_u, subnormal -- would need the chain itself: minutes of numpy);
# they are also the cases with NaN and infinite columns in several item ranges, what the shared bounds of a split launch are about
SPLIT_CASES = ('nan_in', 'nan_u', 'inf_in')
NAN_PATTERNS = (0x7fc00000, 0xffc00000, 0x7fffffff, 0xffc00001)
SHORT_ROW, EMPTY_ROW = 5, 7                  # keeps 3 columns / keeps none
ZERO_ROWS = (11, 70)                         # user rows of zeros: 0 * inf, -0.0 products
CASES = ('nan_in', 'nan_u', 'inf_in', 'overflow', 'huge_u', 'tiny_u', 'subnormal')
SEED = 8800


def nan32(pattern):
    return np.array([pattern], dtype=np.uint32).view(F32)[0]


def special_cols(n_cols):
    """eight columns: first tile, both sides of a tile edge, the middle, the last tile and the last column (several item ranges of a
    split catalogue)"""
    return [3, 31, 32, n_cols // 3, n_cols // 3 + 1, (2 * n_cols) // 3, n_cols - (n_cols % 32 or 32), n_cols - 1]


def _base(rng, n_rows, n_cols, k):
    U = rng.integers(-3, 4, (n_rows, k)).astype(F32)
    V = rng.integers(-20, 21, (n_cols, k)).astype(F32)
    b = rng.integers(-8, 9, n_cols).astype(F32)
    for r in ZERO_ROWS:
        U[r] = 0
    return U, V, b


def _rated(rng, n_rows, n_cols, sc):
    """about 40 rated columns per row; by row % 4: every special column rated / the first half of them / as drawn / none of them"""
    rated = []
    for r in range(n_rows):
        cols = set(int(c) for c in rng.choice(n_cols, int(rng.integers(30, 51)), replace=False))
        if r % 4 == 0:
            cols |= set(sc)
        elif r % 4 == 1:
            cols = (cols - set(sc)) | set(sc[:4])
        elif r % 4 == 3:
            cols -= set(sc)
        rated.append(cols)
    keep = [sc[1], sc[4], int(rng.integers(40, 90))]             # the short row keeps two special columns and an ordinary one
    rated[SHORT_ROW] = set(range(n_cols)) - set(keep)
    rated[EMPTY_ROW] = set(range(n_cols))
    return [np.array(sorted(x), dtype=np.int32) for x in rated]


@functools.lru_cache(maxsize=None)
def case(name, k, shape=None):
    """-> dict(U, V, b, rated, special): the input set `name` at factor width k ((N_ROWS, N_COLS) unless shape says otherwise)"""
    n_rows, n_cols = shape or (N_ROWS, N_COLS)
    rng = np.random.Generator(np.random.PCG64(SEED + 131 * CASES.index(name) + k + n_cols))
    U, V, b = _base(rng, n_rows, n_cols, k)
    sc = special_cols(n_cols)
    j = [int(x) for x in rng.permutation(k)[:8]] if k >= 8 else [0] * 8
    kh = (k + 1) // 2
    if name == 'nan_in':                                         # one NaN in each special item row, two user rows with a NaN
        for i, c in enumerate(sc):
            V[c, j[i]] = nan32(NAN_PATTERNS[i % 4])
        U[3, j[0]] = nan32(NAN_PATTERNS[2])
        U[n_rows - 1, j[1]] = nan32(NAN_PATTERNS[1])
    elif name == 'nan_u':                                        # finite items: a few users only are NaN or infinite
        U[3, j[0]] = nan32(NAN_PATTERNS[3])
        U[n_rows - 1, j[1]] = nan32(NAN_PATTERNS[0])
        U[40, j[2]] = np.inf
        V[sc[0], j[2]] = 0                                       # 0 * inf
        U[41, j[3]] = -np.inf
    elif name == 'inf_in':
        ja, jb = j[0], j[1]
        U[:, ja] = np.where(U[:, ja] == 0, 1, U[:, ja])          # u != 0 at ja except the rows below
        U[0::5, ja] = 0                                          # u == 0 meets inf: NaN
        U[ZERO_ROWS[0]] = 0
        U[SHORT_ROW, ja] = -1                                    # the short row keeps a -inf column
        U[SHORT_ROW, jb] = 1
        for c in sc[:3]:
            V[c, ja] = np.inf                                    # three columns tie at +inf (u > 0) or at -inf (u < 0)
        V[sc[3], ja] = -np.inf
        V[sc[4], ja] = np.inf                                    # sc[4] is kept by the short row: -inf there
        V[sc[5], ja], V[sc[5], jb] = np.inf, -np.inf             # both signs in one chain
        V[sc[6], ja], V[sc[6], jb] = np.inf, np.inf
        V[sc[7], jb] = -np.inf
        V[sc[1], jb] = 0                                         # (sc[1], kept by the short row too: +inf * -1 alone decides)
        V[sc[4], jb] = 0
    elif name == 'overflow':                                     # finite factors: +-2^100 at one step of each k-half (the SAME
        ja = j[0] % kh                                           # MFMA when k is even) and at a third
        jb = min(ja + kh, k - 1)
        jc = (ja + 1) % kh
        big = F32(2.0 ** 100)
        for col in (ja, jb, jc):
            U[:, col] = 0
            V[:, col] = 0
        U[1::3, ja] = big
        U[2::3, ja] = -big
        U[1::4, jb] = -big
        U[2::7, jc] = big
        for r in ZERO_ROWS:
            U[r] = 0
        V[sc[0], ja] = V[sc[1], ja] = V[sc[2], ja] = big          # ties at +inf and at -inf
        V[sc[3], ja] = -big
        V[sc[4], ja], V[sc[4], jb] = big, big                    # 2^200 then -2^200 in one chain: the first decides
        V[sc[5], jb], V[sc[5], jc] = -big, big
        jd = (ja + 2) % kh                                       # the bias add overflows: +-2^127 + 3e38
        U[:, jd] = np.where(np.arange(n_rows) % 2 == 0, F32(2.0 ** 63), F32(-2.0 ** 63))
        U[0::9, jd] = 0
        V[:, jd] = 0
        V[sc[6], jd] = V[sc[7], jd] = F32(2.0 ** 64)
        b[sc[6]], b[sc[7]] = F32(3e38), F32(-3e38)
    elif name == 'huge_u':                                       # sum u^2 overflows; every score is ordinary
        U, V, b = U * F32(2.0 ** 70), V * F32(2.0 ** -80), b * F32(2.0 ** -10)
    elif name == 'tiny_u':                                       # sum u^2 underflows to 0
        U, V, b = U * F32(2.0 ** -80), V * F32(2.0 ** 60), b * F32(2.0 ** -20)
    elif name == 'subnormal':                                    # every score an exact multiple of 2^-149 below 2^-126
        U, V, b = U * F32(2.0 ** -70), V * F32(2.0 ** -79), b * F32(2.0 ** -149)
        for c in sc[:4]:
            V[c], b[c] = 0, 0                                    # exact zeros
        V[sc[4]], b[sc[4]] = -np.abs(V[sc[4]]) - F32(2.0 ** -79), 0   # all negative: -0.0 products for the rows of zeros
        V[sc[5]], b[sc[5]] = V[sc[4]], 0
    else:
        raise KeyError(name)
    rated = _rated(rng, n_rows, n_cols, sc)
    return dict(U=np.ascontiguousarray(U, dtype=F32), V=np.ascontiguousarray(V, dtype=F32), b=np.ascontiguousarray(b, dtype=F32),
                rated=rated, special=sc)


@functools.lru_cache(maxsize=None)
def scores(name, k):
    """the chain's scores of case(name, k): the specification, overflow included"""
    c = case(name, k)
    with np.errstate(all='ignore'):
        s = R.mfma_chain_scores(c['U'], c['V'], c['b'])
    s.setflags(write=False)
    return s


def split_scores(c):
    """the chain's scores of an integer-factor case without walking the chain over the whole table: where a user row and an item row
    are finite the score is an exact integer (one float64 matrix product), everything else -- the rows and columns that hold a NaN or
    an infinity -- goes through R.mfma_chain_scores.  tests/test_nonfinite_cpu.py holds it to the chain at the small shape."""
    U, V, b = c['U'], c['V'], c['b']
    s = (U.astype(np.float64) @ V.astype(np.float64).T + b.astype(np.float64)).astype(F32) + F32(0.0)
    rows = np.flatnonzero(~np.isfinite(U).all(axis=1))
    cols = np.flatnonzero(~np.isfinite(V).all(axis=1))
    with np.errstate(all='ignore'):
        if len(rows):
            s[rows] = R.mfma_chain_scores(U[rows], V, b)
        if len(cols):
            s[:, cols] = R.mfma_chain_scores(U, V[cols], b[cols])
    return s


@functools.lru_cache(maxsize=None)
def split_case(name):
    n_rows, n_cols, k = SPLIT
    c = dict(case(name, k, (n_rows, n_cols)))
    with np.errstate(all='ignore'):
        c['scores'] = split_scores(c)
    return c


# ---- the contract, stated without argsort ---------------------------------------------------------------------------------------------
def contract_order(scores_row):
    """every column of the row, best first: sorted by (is NaN, score, column), descending"""
    s = np.asarray(scores_row)
    keys = [(bool(np.isnan(s[c])), 0.0 if np.isnan(s[c]) else float(s[c]), c) for c in range(len(s))]
    return [c for _, _, c in sorted(keys, reverse=True)]


def likes_of(scores_row, rated, listed):
    """the likes of a row for K8: the columns of its top list `listed` (-1 padding ignored), its first 64 NaN / +inf / -inf columns,
    its first five rated columns -> sorted unique int32"""
    s = np.asarray(scores_row)
    out = set(int(c) for c in listed if c >= 0)
    out |= set(int(c) for c in np.flatnonzero(~np.isfinite(s))[:64])
    out |= set(int(c) for c in np.asarray(rated)[:5])
    return np.array(sorted(out), dtype=np.int32)


def same_scores(got, want):
    """bit equality where `want` is not NaN, NaN where it is (the payload of a NaN is not specified)"""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
