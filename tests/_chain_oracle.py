"""The score chain of oracle/ref_np.mfma_chain_scores with its one weakness marked, and the inputs of tests/test_gpu_score_chain.py.

mfma_chain_scores rounds every step twice -- the float64 sum of the exact product and the accumulator, then float32 -- where the
hardware's fused multiply-add rounds once.  The two differ only when the float64 sum was inexact AND landed exactly on a float32
rounding tie; chain_scores_checked marks those entries (`hazard`), so a test can ask for bit equality everywhere else without a share
of allowed mismatches.  exact_chain_score is the same chain in integer arithmetic, one rounding per step: the proof of the marking.
Not a test module."""
import numpy as np

from oracle import ref_np as R

F32 = np.float32
_LOW29 = np.uint64((1 << 29) - 1)
_TIE29 = np.uint64(1 << 28)
_F32_MIN_NORMAL = 2.0 ** -126
_PRODUCT_FLOOR = 2.0 ** -960                 # a 48-bit product below this may have lost bits to float64's subnormal range


def _twosum_inexact(a, b, s):
    """True where the float64 sum s = fl(a + b) is not a + b (Knuth's TwoSum: the error term is exact)"""
    bb = s - a
    return ((a - (s - bb)) + (b - bb)) != 0.0


def chain_scores_checked(U, V, bias=None, order='global', chunk=1 << 17):
    """-> (scores float32 [rows, cols], hazard bool [rows, cols]).  scores: R.mfma_chain_scores(U, V, bias), bit for bit.  hazard: some
    step of the entry's chain gave a float64 sum that was inexact and sits exactly on a float32 rounding tie (the 29 bits float32 drops
    are 1 0...0), or is not exact and lies in float32's subnormal range, or its product may have underflowed float64: everywhere else
    two roundings equal one.  The bias add is a float32 add on both sides: one rounding, never a hazard.
    order: 'global' -- halves of ceil(k / 2), the chain of the library; 'slabs' -- the halves interleaved inside every 256 factors, the
    order score_topk_slab_kernel ran before it was held to the global chain (kept so the inputs can be shown to tell the two apart)."""
    U, V = np.ascontiguousarray(U, dtype=F32), np.ascontiguousarray(V, dtype=F32)
    k = U.shape[1]
    steps = chain_order(k, order)
    u64 = U.astype(np.float64)
    scores = np.empty((U.shape[0], V.shape[0]), dtype=F32)
    hazard = np.zeros(scores.shape, dtype=bool)
    step_cols = max(1, chunk // max(1, U.shape[0]))
    for c0 in range(0, V.shape[0], step_cols):
        v64 = V[c0:c0 + step_cols].astype(np.float64)
        acc = np.zeros((U.shape[0], v64.shape[0]), dtype=F32)
        hz = np.zeros(acc.shape, dtype=bool)
        p, s, mag = np.empty(acc.shape, dtype=np.float64), np.empty(acc.shape, dtype=np.float64), np.empty(acc.shape, dtype=F32)
        low, cand = np.empty(acc.shape, dtype=np.uint64), np.empty(acc.shape, dtype=bool)
        for j in steps:
            np.multiply(u64[:, j:j + 1], v64[:, j].reshape(1, -1), out=p)
            np.add(p, acc, out=s)
            np.bitwise_and(s.view(np.uint64), _LOW29, out=low)
            np.equal(low, _TIE29, out=cand)
            # the two rare ranges: looked for entry by entry only in a step whose smallest magnitude reaches them (an exact 0 does)
            nxt = s.astype(F32)
            if np.abs(nxt, out=mag).min() <= _F32_MIN_NORMAL:          # (a sum below 2^-126 rounds to at most 2^-126)
                cand |= (np.abs(s) < _F32_MIN_NORMAL) & (s != 0.0)
            if np.abs(u64[:, j]).min() * np.abs(v64[:, j]).min() < _PRODUCT_FLOOR:      # the smallest |product| of the step
                cand |= (np.abs(p) < _PRODUCT_FLOOR) & (p != 0.0)
            if cand.any():
                at = np.nonzero(cand)
                a64 = acc[at].astype(np.float64)
                bad = _twosum_inexact(p[at], a64, s[at]) | (np.abs(p[at]) < _PRODUCT_FLOOR)
                hz[at[0][bad], at[1][bad]] = True
            acc = nxt
        if bias is not None:
            acc = (acc + np.asarray(bias, dtype=F32)[c0:c0 + step_cols].reshape(1, -1)).astype(F32)
        scores[:, c0:c0 + step_cols] = acc + F32(0.0)
        hazard[:, c0:c0 + step_cols] = hz
    return scores, hazard


def chain_order(k, order='global'):
    """the factor indices in the order the chain adds their products"""
    if order == 'global':
        kh = (k + 1) // 2
        out = []
        for j in range(kh):
            out.append(j)
            if kh + j < k:
                out.append(kh + j)
        return out
    assert order == 'slabs'
    out = []
    for s0 in range(0, k, 256):
        for kk in range(128):
            for e in (s0 + kk, s0 + 128 + kk):
                if e < k:
                    out.append(e)
    return out


# ---- the same chain in exact integer arithmetic --------------------------------------------------------------------------------
def _dyadic(x):
    """float -> (n, e) with x == n * 2^e exactly"""
    num, den = float(x).as_integer_ratio()
    return num, -(den.bit_length() - 1)


def round_to_f32(n, e):
    """the float32 nearest to n * 2^e (n, e integers), ties to even, subnormals included -> (n', e') with at most 24 bits in n'"""
    if n == 0:
        return 0, 0
    sign, a = (-1 if n < 0 else 1), abs(n)
    shift = max(a.bit_length() - 24, -149 - e)
    if shift <= 0:
        return n, e
    q, r = divmod(a, 1 << shift)
    half = 1 << (shift - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return sign * q, e + shift


def exact_chain_score(u, v, bias=None, order='global'):
    """one entry of the chain, every fma rounded ONCE from its exact value -> np.float32"""
    n, e = 0, 0
    for j in chain_order(len(u), order):
        (a, ea), (b, eb) = _dyadic(u[j]), _dyadic(v[j])
        pn, pe = a * b, ea + eb
        lo = min(pe, e)
        n, e = round_to_f32(pn * (1 << (pe - lo)) + n * (1 << (e - lo)), lo)
    if bias is not None:
        bn, be = _dyadic(bias)
        lo = min(be, e)
        n, e = round_to_f32(bn * (1 << (be - lo)) + n * (1 << (e - lo)), lo)
    return F32(np.ldexp(float(n), e)) + F32(0.0)


# ---- the inputs of tests/test_gpu_score_chain.py ---------------------------------------------------------------------------------
# k: 1, 3, 129, 255, 256 -- the plain fp32-MFMA kernel, odd widths, the widest single tile; 257 -- the first slab width, scalar staging;
# 264 -- k % 8 == 0, vector staging and exact_score's aligned path; 300 -- k % 4 == 0 but not % 8; 387, 512 -- two slabs; 513 -- three;
# 768 -- the last slab width; 769, 1032 -- the generic wave-per-row kernel
WIDTHS = [1, 3, 129, 255, 256, 257, 264, 300, 387, 512, 513, 768, 769, 1032]
SLAB_WIDTHS = [k for k in WIDTHS if 256 < k <= 768]
N_ROWS, N_COLS, TOP = 130, 333, 30           # two user blocks of 128 with a tail; a tail tile
N_USERS_ALL = 150                            # the table user_idx gathers from (k = 387)
IDX_WIDTH = 387
BIG = (40, 66000, 258)                       # the 32-bit column-id instantiation of the slab kernel
SEED = 7100


def generic(seed, n_rows, n_cols, k):
    """N(0, 0.01^2) factors and biases rounded like '%f', 0 to 59 rated columns per row: tests/test_gpu_candidates._generic"""
    rng = np.random.Generator(np.random.PCG64(seed))
    U = np.round(rng.standard_normal((n_rows, k)) * 0.01, 6).astype(np.float32)
    V = np.round(rng.standard_normal((n_cols, k)) * 0.01, 6).astype(np.float32)
    b = np.round(rng.standard_normal(n_cols) * 0.01, 6).astype(np.float32)
    rated = [np.sort(rng.choice(n_cols, int(rng.integers(0, 60)), replace=False)).astype(np.int32) for _ in range(n_rows)]
    return rng, U, V, b, rated


def case(k, shape=None):
    """-> dict(U, V, b, rated, user_idx, rows): the input set of width k.  user_idx is None except at k = 387 (a permutation of a larger
    table, one user twice); `rows` is U[user_idx] (or U): the factor rows the lists are of."""
    n_rows, n_cols = shape or (N_ROWS, N_COLS)
    with_idx = shape is None and k == IDX_WIDTH
    rng, U, V, b, rated = generic(SEED + k, N_USERS_ALL if with_idx else n_rows, n_cols, k)
    idx = None
    if with_idx:
        idx = rng.permutation(N_USERS_ALL)[:n_rows].astype(np.int32)
        idx[-1] = idx[0]
        rated = rated[:n_rows]
    return dict(U=U, V=V, b=b, rated=rated, user_idx=idx, rows=U if idx is None else U[idx])


# ---- near-ties by construction: the inputs of the K6 tests (tests/test_gpu_utils_eval.py) and of the mirror case of the chain file -----
# widths of tkr_raw_ranks: one factor; an odd width below a wave; 50 (the first width the near-ties show at); 64 / 65, 128 / 129 and
# 256 / 257 -- one more 64-wide pass of the reduction K6 had; 200; 300, 387, 513 -- above the 256 K6 stopped at, K4's slab kernel; 769,
# 1032 -- K4's generic kernel
MIRROR_WIDTHS = [1, 7, 50, 64, 65, 128, 129, 200, 256, 257, 300, 387, 513, 769, 1032]
MIRROR_ROWS, MIRROR_M = 62, 600              # 15 blocks of 4 waves and a tail of 2; 1,200 columns, rated rows of ~600: ten waves long
MIRROR_SEED = 9100


def mirror_case(k, n_rows=MIRROR_ROWS, m=MIRROR_M, seed=None):
    """-> dict(U, V, b, rated, user_idx, rows) as case(): a catalogue of m mirror pairs.  The user rows are palindromes (U[r, j] ==
    U[r, k-1-j]; at odd k the middle factor is free), column c + m is column c read backwards with the same bias: the two scores of a
    pair are equal in real arithmetic and only the order of summation separates them in fp32.  Values are N(0, 0.01^2) rounded like
    '%f'.  Every column is rated with probability 1/2 on its own, so half the pairs have exactly one column rated; row 0 has no rated
    column, row 1 all but 3 (its kept list is shorter than any K > 3), row 2 every column.  At k = IDX_WIDTH user_idx is a permutation
    of a larger table with one user twice."""
    seed = MIRROR_SEED + k if seed is None else seed
    rng = np.random.Generator(np.random.PCG64(seed))
    with_idx = k == IDX_WIDTH
    n_all = n_rows + 20 if with_idx else n_rows
    half = (k + 1) // 2
    A = np.round(rng.standard_normal((n_all, half)) * 0.01, 6).astype(F32)
    U = np.empty((n_all, k), dtype=F32)
    U[:, :half] = A
    U[:, k - half:] = A[:, ::-1]
    V0 = np.round(rng.standard_normal((m, k)) * 0.01, 6).astype(F32)
    b0 = np.round(rng.standard_normal(m) * 0.01, 6).astype(F32)
    V = np.ascontiguousarray(np.concatenate([V0, V0[:, ::-1]]))
    b = np.concatenate([b0, b0])
    rated = [np.flatnonzero(rng.random(2 * m) < 0.5).astype(np.int32) for _ in range(n_rows)]
    if n_rows > 0:
        rated[0] = np.zeros(0, dtype=np.int32)
    if n_rows > 1:
        rated[1] = np.delete(np.arange(2 * m, dtype=np.int32), np.sort(rng.choice(2 * m, 3, replace=False)))
    if n_rows > 2:
        rated[2] = np.arange(2 * m, dtype=np.int32)
    idx = None
    if with_idx:
        idx = rng.permutation(n_all)[:n_rows].astype(np.int32)
        idx[-1] = idx[3]                     # (rows 0 to 2 keep their special rated lists to themselves)
    return dict(U=U, V=V, b=b, rated=rated, user_idx=idx, rows=U if idx is None else U[idx])


def left_to_right_scores(U, V, bias=None):
    """the same products added in plain index order, one fp32 rounding per step (the double rounding of mfma_chain_scores, unmarked):
    a second summation order, to show that an input set tells orders apart.  Not an oracle of any kernel."""
    u64, v64 = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    acc = np.zeros((u64.shape[0], v64.shape[0]), dtype=F32)
    for j in range(u64.shape[1]):
        acc = (np.outer(u64[:, j], v64[:, j]) + acc).astype(F32)
    if bias is not None:
        acc = (acc + np.asarray(bias, dtype=F32).reshape(1, -1)).astype(F32)
    return acc + F32(0.0)
