"""The fp16 pass of K4's bound-and-refine arithmetic restated on the CPU, its documented margin, and inputs built to sit near it.

csrc/topk_parts.h refine_prologue (derived above score_topk_bf16_kernel in csrc/topk.hip) promises, in a user's scaled units,

    |approx - exact| <= margin = scale * (1.05 * 2^-10 * |u| * max|v_i| + 2^-18 * (|u| * max|v_i| + max|bias|)) + 2.01 * KPAD

and the candidate lists keep everything within 2 * margin of the K-th best approximate score.  Random factors use a few per cent of
that margin, so a filter that kept 1 * margin, or a coefficient of 2^-11, would pass every test on random inputs.  adversarial_case
builds inputs on which every fp16 rounding pushes one item (the victim: first by exact score) DOWN and at least K others (the decoys:
just behind it by exact score) UP, so that the victim lies about 0.8 of 2 * margin below the K-th best approximate score.

The conditions of the construction are checked on the CPU by tests/test_topk_margin_cpu.py; tests/test_gpu_topk_margin.py runs the
kernels on the same cases (CASES, SPLIT_CASES, FIRST_FORM_CASES below).  Not a test module."""
import numpy as np

from oracle import ref_np as R

F32 = np.float32
DELTA = 2.0 ** -11            # half an ulp of fp16 at 1


def pow2_scale(amax):
    """2^e with amax * 2^e in [2^13, 2^14) (1 for amax = 0): csrc/topk_parts.h pow2_scale, without its clamp"""
    amax = np.asarray(amax, dtype=np.float64)
    e = np.floor(np.log2(np.where(amax > 0, amax, 1.0)))
    return np.where(amax > 0, 2.0 ** (13 - e), 1.0)


def scales(U, V):
    """-> (su [rows], sv): the powers of two of the fp16 pass"""
    return pow2_scale(np.abs(U).max(axis=1)), float(pow2_scale(np.abs(V).max()))


def approx_scores(U, V, bias=None):
    """The fp16 pass in the user's scaled units: factors scaled by su (per row) / sv (the table), rounded through np.float16 (round to
    nearest even, as the device cast), products summed in float64, plus bias * su * sv.  -> (scores [rows, cols], scale [rows])"""
    U, V = np.asarray(U, dtype=F32), np.asarray(V, dtype=F32)
    su, sv = scales(U, V)
    with np.errstate(over='ignore'):
        hu = (U.astype(np.float64) * su[:, None]).astype(np.float16).astype(np.float64)
        hv = (V.astype(np.float64) * sv).astype(np.float16).astype(np.float64)
    s = hu @ hv.T
    scale = su * sv
    if bias is not None:
        s = s + np.asarray(bias, dtype=np.float64)[None, :] * scale[:, None]
    return s, scale


def margin(U, V, bias, k):
    """The documented margin per row, float64, in the row's scaled units; KPAD = 16 * ceil(k / 16)"""
    U64, V64 = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    su, sv = scales(U, V)
    reach = np.sqrt((U64 * U64).sum(axis=1)) * np.sqrt((V64 * V64).sum(axis=1)).max()
    bmax = 0.0 if bias is None else float(np.abs(np.asarray(bias, dtype=np.float64)).max())
    kpad = 16 * ((k + 15) // 16)
    return su * sv * (1.05 * 2.0 ** -10 * reach + 2.0 ** -18 * (reach + bmax)) + 2.01 * kpad


def key16_edge(x, bits=16):
    """the smallest float32 with the upper `bits` bits of x (x > 0).  The packed lists of the second form hold a score as its upper
    16 bits, and the finish kernel cuts at the 16-bit key of the bound; the scheduled trim (csrc/topk_refine.hip trim_all2) searches
    the K-th best key among 15-bit keys -- while the threshold is still below zero and the scores above, the keys lie on both sides
    of zero: it keeps the sign bit and drops the lowest -- so the K-th best score is known to it as the edge of its 15-bit key"""
    b = np.asarray(x, dtype=F32).view(np.uint32) & np.uint32((0xffffffff << (32 - bits)) & 0xffffffff)
    return b.view(F32).astype(np.float64)


def key16_width(x, bits=16):
    """distance from key16_edge(x, bits) to the next key's edge (x > 0)"""
    b = (np.asarray(x, dtype=F32).view(np.uint32) & np.uint32((0xffffffff << (32 - bits)) & 0xffffffff)) + np.uint32(1 << (32 - bits))
    return b.view(F32).astype(np.float64) - key16_edge(x, bits)


def adversarial_case(k, K, n_rows=130, n_cols=320, n_decoys=40, seed=0, bias=False, rated_decoys=0, first_tile=0, victim_tile=None,
                     e_lo=-40, e_hi=40, gap=0.05, step=0.002):
    """-> dict(U, V, bias, rated, victim, decoys, k, K).

    Coordinates: one common coordinate z and the others cut into halves A and B at random; a random sign per coordinate on the user
    and every item alike (products keep their sign).  Per user, a = 2^e (e spread over [e_lo, e_hi]: every user its own su), c = 2^-3:
      user     u_A = a (1 + 0.98 d), u_B = a (1 + 1.02 d), d = 2^-11: in fp16 |u_A| rounds down by almost half an ulp, |u_B| up
      victim   v_A = +c (1 + 0.98 d), v_B = -(c/2) (1 + 1.02 d): every product's rounding lowers the approximate score
      decoys   v_A = -(c/2) (1 + 0.98 d), v_B = +c (1 + 1.02 d): every rounding raises it; decoy q's EXACT score is put
               (gap + step q) * 2^-10 * sum|terms| below the victim's through one adjuster: one B coordinate, or (bias=True) its bias
      fillers  N(0, 0.01^2)
    z: u_z = a, v_z = r for victim and decoys alike, both exact in fp16 -- it adds the same amount to their exact and approximate
    scores and no rounding.  r is chosen so that the decoys' approximate scores sit just above an edge of the 15-bit keys
    (key16_edge(x, 15)): the trim knows a K-th best score only as the lower edge of its key, up to 2^-6 relative below it, which is more
    than 2 * margin here (~0.65 % of the score) -- without the alignment a kernel that kept 1 * margin could pass by that slack.
    The victim and the decoys fill columns of tiles first_tile and first_tile + 1 (victim_tile: the victim alone goes there), spread
    over both half-lane groups (columns c with c % 8 < 4 and >= 4).  bias=True: one exponent for all users (a bias is per item).
    rated_decoys: every third user has that many decoys rated."""
    rng = np.random.Generator(np.random.PCG64(seed * 1000 + k))
    assert k >= 3 and n_decoys >= K + rated_decoys and (first_tile + 2) * 32 <= n_cols
    perm = rng.permutation(k)
    z, rest = perm[0], perm[1:]
    A, B = rest[:(k - 1) // 2], rest[(k - 1) // 2:]
    sign = rng.choice([-1.0, 1.0], k)
    if bias:
        e = np.full(n_rows, int(rng.integers(-3, 4)))
    else:
        e = np.round(np.linspace(e_lo, e_hi, n_rows)).astype(int)
        rng.shuffle(e)
    a = 2.0 ** e.astype(np.float64)
    c = 2.0 ** -3
    pu = np.zeros(k)
    pu[A], pu[B], pu[z] = 1 + 0.98 * DELTA, 1 + 1.02 * DELTA, 1.0
    U = (a[:, None] * (pu * sign)[None, :]).astype(F32)
    vic = np.zeros(k)
    vic[A], vic[B] = c * (1 + 0.98 * DELTA), -(c / 2) * (1 + 1.02 * DELTA)
    dec = np.zeros(k)
    dec[A], dec[B] = -(c / 2) * (1 + 0.98 * DELTA), c * (1 + 1.02 * DELTA)
    vic, dec = (vic * sign).astype(F32), (dec * sign).astype(F32)

    V = (rng.standard_normal((n_cols, k)) * 0.01).astype(F32)
    b = np.zeros(n_cols, dtype=F32) if bias else None
    if bias:
        b[:] = (rng.standard_normal(n_cols) * 1e-4).astype(F32)
    # columns: the special block in two tiles, balanced over the half-lane groups
    block = np.arange(first_tile * 32, first_tile * 32 + 64)
    lo, hi = block[block % 8 < 4], block[block % 8 >= 4]
    n_special = n_decoys + (1 if victim_tile is None else 0)
    pick = np.concatenate([rng.permutation(lo)[:(n_special + 1) // 2], rng.permutation(hi)[:n_special // 2]])
    rng.shuffle(pick)
    if victim_tile is None:
        victim, decoys = int(pick[0]), pick[1:]
    else:
        victim, decoys = int(victim_tile * 32 + rng.integers(0, 32)), pick
        assert victim < n_cols and victim not in set(decoys.tolist())
    V[victim] = vic
    V[decoys] = dec
    if b is not None:
        b[victim] = 0.0
        b[decoys] = 0.0

    # the adjusters: exact scores of unit user (a = 1), float64 from the float32 values
    u1 = (U[0].astype(np.float64) / a[0])
    terms = np.abs(u1 * V[victim].astype(np.float64)).sum()
    s_vic = float(u1 @ V[victim].astype(np.float64))
    for q, col in enumerate(decoys):
        target = s_vic - (gap + step * q) * 2.0 ** -10 * terms
        if bias:
            b[col] = F32((target - float(u1 @ V[col].astype(np.float64))) * a[0])
        else:
            j = B[q % len(B)]
            others = float(u1 @ V[col].astype(np.float64)) - u1[j] * float(V[col, j])
            V[col, j] = F32((target - others) / u1[j])

    # the common coordinate: lift the decoys' approximate scores to just above a 16-bit key edge
    special = np.concatenate([[victim], decoys])
    ap, _ = approx_scores(U[:1], V[special], None if b is None else b[special])
    d_min = ap[0, 1:].min()
    edge = key16_edge(d_min, 15)
    width = key16_width(d_min, 15)
    off = (edge + width) * (1 + 2.0 ** -13) - d_min if d_min - edge > 0.02 * width else 0.0
    su0, sv = scales(U[:1], V)
    r_scaled = float(np.float16(off / (float(su0[0]) * abs(U[0, z])))) if off else 0.0           # fp16-exact in the table's scaled units
    V[special, z] = F32(r_scaled / sv * sign[z])
    assert float(pow2_scale(np.abs(V).max())) == sv

    rated = [[] for _ in range(n_rows)]
    if rated_decoys:
        for r in range(0, n_rows, 3):
            rated[r] = sorted(int(x) for x in rng.choice(decoys, rated_decoys, replace=False))
            rated[r] += sorted(int(x) for x in rng.choice(np.setdiff1d(np.arange(n_cols), special), 5, replace=False))
    return dict(U=U, V=V, bias=b, rated=rated, victim=victim, decoys=[int(x) for x in decoys], k=k, K=K, n_rows=n_rows, n_cols=n_cols)


def case_conditions(case, rows=None):
    """What the construction promises, measured: -> dict of per-case figures over `rows` (default: all).
      victim_exact_rank  worst rank of the victim among the unrated columns by oracle/ref_np.mfma_chain_scores (0 = first)
      cut_tie            an exact tie between the K-th and (K+1)-th chain score of some row
      victim_approx_rank smallest number of unrated columns whose approximate score is above the victim's
      share              smallest (K-th best approximate score - victim's) / (2 * margin)
      used               largest |approx - exact| / margin over all items
      align              largest (K-th best approximate score - the edge of its 15-bit key) / (2 * margin)
      key_drop_1m        in every row key16(victim) < key16(edge of the K-th score's 15-bit key - margin): the second form drops an
                         entry of a list only by its key (csrc/topk_refine.hip trim_all2, and topk_finish2_kernel at the 16-bit key of
                         the bound the trim found), so this is what makes a filter of 1 * margin LOSE the victim there; share > 0.5
                         alone does not
      key_keep_2m        in every row key16(victim) >= key16(that edge - 2 * margin): the documented filter keeps it
      key_width          largest width of the K-th score's key / margin"""
    U, V, b, K, k = case['U'], case['V'], case['bias'], case['K'], case['k']
    rows = range(len(U)) if rows is None else rows
    chain = R.mfma_chain_scores(U, V, b)
    ap, scale = approx_scores(U, V, b)
    m = margin(U, V, b, k)
    out = dict(victim_exact_rank=0, cut_tie=False, victim_approx_rank=10 ** 9, share=np.inf, used=0.0, align=0.0, key_drop_1m=True,
               key_keep_2m=True, key_width=0.0)
    out['used'] = float((np.abs(ap - chain.astype(np.float64) * scale[:, None]) / m[:, None]).max())
    for r in rows:
        keep = np.ones(V.shape[0], bool)
        keep[case['rated'][r]] = False
        ex, apx = chain[r][keep], ap[r][keep]
        assert keep[case['victim']]
        v_at = int(keep[:case['victim']].sum())
        order = np.sort(ex)[::-1]
        out['victim_exact_rank'] = max(out['victim_exact_rank'], int((ex > ex[v_at]).sum()))
        out['cut_tie'] |= bool(order[K - 1] == order[K])
        out['victim_approx_rank'] = min(out['victim_approx_rank'], int((apx > apx[v_at]).sum()))
        kth = np.sort(apx)[::-1][K - 1]
        out['share'] = min(out['share'], float((kth - apx[v_at]) / (2 * m[r])))
        edge, vkey = key16_edge(kth, 15), key16_edge(apx[v_at])
        out['align'] = max(out['align'], float((kth - edge) / (2 * m[r])))
        out['key_drop_1m'] &= bool(vkey < key16_edge(edge - m[r]))
        out['key_keep_2m'] &= bool(vkey >= key16_edge(edge - 2 * m[r]))
        out['key_width'] = max(out['key_width'], float(key16_width(kth) / m[r]))
    return out


def generic_inputs(n_rows, n_cols, k, bias, wide):
    """the inputs of tests/test_gpu_topk.py test_refine_is_the_fp32_arithmetic (same generator, same order of draws)"""
    rng = np.random.Generator(np.random.PCG64(n_rows + 3 * n_cols + k))
    U = (rng.standard_normal((n_rows, k)) * 0.01).astype(F32)
    V = (rng.standard_normal((n_cols, k)) * 0.01).astype(F32)
    if wide:
        U *= (10.0 ** rng.uniform(-4, 5, (n_rows, 1))).astype(F32)
        V *= (10.0 ** rng.uniform(-5, 4, (n_cols, k))).astype(F32)
    b = (rng.standard_normal(n_cols) * 0.002).astype(F32) if bias else None
    return U, V, b


GENERIC_SHAPES = [(300, 2000, 128, True, False), (1000, 700, 64, False, False), (513, 1500, 100, True, False), (200, 900, 50, True, True),
                  (3000, 5000, 128, True, False), (64, 70000, 32, False, False)]


# ---- the cases tests/test_gpu_topk_margin.py runs and tests/test_topk_margin_cpu.py checks ------------------------------------------
# Catalogues of 10 to 13 tiles: the plan of 130 rows cuts them into item ranges of two tiles (csrc/topk.hip pick_splits), and the
# victim and its decoys fill ONE range (tiles 2j, 2j + 1), where at least K decoys meet in one list and set its threshold.
def _variants(k, i):
    n_cols = (320, 333, 390, 352)[i % 4]
    last_pair = (n_cols // 32) // 2 - 1
    return [dict(k=k, K=30, n_cols=n_cols, bias=False, rated_decoys=5, first_tile=2 * ((i + 1) % (last_pair + 1)), seed=1),
            dict(k=k, K=30, n_cols=n_cols, bias=True, rated_decoys=0, first_tile=2 * ((i + 2) % (last_pair + 1)), seed=2),
            dict(k=k, K=8, n_cols=n_cols, bias=True, rated_decoys=5, first_tile=2 * (i % (last_pair + 1)), seed=3),
            dict(k=k, K=1, n_cols=n_cols, bias=False, rated_decoys=0, first_tile=2 * last_pair, seed=4)]


# KS = 1, 2, 4, 8; k % 4 != 0 (50: the scalar staging), odd k (15, 119).  The odd widths are chosen, not arbitrary: the second form
# drops a list entry only by its 16-bit key (case_conditions, key_drop_1m), and a filter that kept 1 * margin can show there only if
# a key edge lies between the victim and (edge of the K-th key - margin) -- necessary; it was not enough.  A key is 2^-7 of its binade wide and the victim sits about
# 1.6 margins below the K-th score, so the keys must be narrower than that: the score, about k / 4 in units of the largest product,
# has to lie in the upper part of its binade.  At k = 15 and 119 a key is 1.3 margins wide; at k = 7 it is 1.48 (and the victim
# 1.44 below), at k = 77 it is 2.0 -- there every list keeps the victim at 1 * margin too, and the cases would assert nothing about
# the factor 2.
SECOND_FORM_WIDTHS = (8, 16, 32, 50, 64, 100, 128, 15, 119)
CASES = [v for i, k in enumerate(SECOND_FORM_WIDTHS) for v in _variants(k, i)]
# thresholds shared across item ranges: one user block, the decoys in the first range and the victim in the last, and the reverse
SPLIT_CASES = [dict(k=k, K=30, n_rows=128, n_cols=640, bias=bias, rated_decoys=rd, first_tile=ft, victim_tile=vt, seed=5 + ft)
               for k in (16, 100) for bias, rd, ft, vt in ((False, 5, 0, 19), (True, 0, 18, 0))]
# the first form: the same cases at two widths, and one catalogue above 65,535 columns (32-bit ids, the work-item table: the
# special tiles lie inside its first span of eight)
FIRST_FORM_CASES = [v for i, k in ((1, 16), (6, 128)) for v in _variants(k, i)]
WIDE_ID_CASE = dict(k=16, K=30, n_rows=33, n_cols=66000, bias=False, rated_decoys=5, first_tile=2, seed=9)


def case_id(p):
    return 'k%d-K%d-n%d-%s-%s-t%d' % (p['k'], p['K'], p['n_cols'], 'bias' if p['bias'] else 'nobias', 'rated' if p['rated_decoys'] else 'free',
                                      p['first_tile'])


def share_floor(k):
    """The share of 2 * margin a case must reach.  0.75, except at the narrowest width: of k = 8 coordinates one is the common
    coordinate (no rounding at all) and one carries a decoy's adjuster (rounded as it falls), so a quarter of the products is not
    adversarial; measured 0.71.  0.7 there -- still well above the 0.5 a 1 * margin filter would survive."""
    return 0.7 if k <= 8 else 0.75


# ---- the GPU side of a case (tests/test_gpu_topk_margin.py and its child process tests/_margin_child.py) -----------------------------
def topk_both_modes(tkr_hip, U, V, b, rated, K, user_idx=None):
    """-> (ids, scores) under 'refine', (ids, scores) under 'fp32', the report of the 'refine' launch"""
    import torch
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n_rows = len(rated)
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(x) for x in rated], out=ptr[1:])
    flat = np.array([c for x in rated for c in sorted(x)], dtype=np.int32)
    mask, pitch = (None, 0) if flat.size == 0 else tkr_hip.build_rated_mask(dev(ptr), dev(flat), n_rows, len(V))
    out = {}
    try:
        for mode in ('refine', 'fp32'):
            tkr_hip.set_topk_math(mode)
            ids, sc = tkr_hip.score_topk(dev(U), dev(V), K, bias=None if b is None else dev(b), mask=mask, mask_pitch=pitch,
                                         user_idx=None if user_idx is None else dev(user_idx.astype(np.int32)), want_scores=True)
            if mode == 'refine':
                report = tkr_hip.topk_last_report()
            else:
                assert tkr_hip.topk_last_report()['form'] == 0
            out[mode] = (ids.cpu().numpy(), sc.cpu().numpy())
    finally:
        tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)
    return out['refine'], out['fp32'], report


def assert_same_as_fp32_and_oracle(refine, fp32, U, V, b, rated, K):
    """ids and score bits under 'refine' are those under 'fp32'; every returned score is the chain oracle's, as
    tests/test_gpu_topk.py test_refine_is_the_fp32_arithmetic holds them (bit for bit but for a 1e-4 fraction -- the float64 double
    rounding of oracle/ref_np.mfma_chain_scores -- and those within rtol 3e-7); and every row's list is the oracle's canonical ranking
    (a row with such a score is left to the first two comparisons)"""
    np.testing.assert_array_equal(refine[0], fp32[0])
    np.testing.assert_array_equal(refine[1].view(np.int32), fp32[1].view(np.int32))
    chain = R.mfma_chain_scores(U, V, b)
    ids, sc = fp32
    listed = ids >= 0
    exp = np.where(listed, np.take_along_axis(chain, np.maximum(ids, 0).astype(np.int64), axis=1), F32(-np.inf))
    same = exp.view(np.int32) == sc.view(np.int32)
    assert same.mean() > 1 - 1e-4
    np.testing.assert_allclose(sc[listed], exp[listed], rtol=3e-7, atol=0)
    for r in range(len(U)):
        ref = R.filtered_topk(chain[r], set(rated[r]), K, canonical=True)
        got = [int(c) for c in ids[r] if c >= 0]
        assert len(got) == len(ref) and np.all(ids[r, len(got):] == -1), 'row %d' % r
        if same[r].all():
            assert got == ref, 'row %d' % r


def run_case_on_gpu(tkr_hip, p, form, image=True, id_bits=16, via_user_idx=False, same_range=True):
    """One adversarial case on the GPU: refine == fp32 == oracle, every victim listed, the report names the form that ran, no block
    was flagged (a flagged block is ranked by the fp32 kernel: the comparison would hold vacuously), and -- same_range -- the plan put
    the special tiles into one item range, where at least K decoys meet."""
    case = adversarial_case(**p)
    U, V, b, rated, K = case['U'], case['V'], case['bias'], case['rated'], case['K']
    user_idx, table = None, U
    if via_user_idx:
        rng = np.random.Generator(np.random.PCG64(p['k']))
        user_idx = rng.permutation(len(U) + 37)[:len(U)]
        table = (rng.standard_normal((len(U) + 37, p['k']))).astype(F32)
        table[user_idx] = U
    refine, fp32, report = topk_both_modes(tkr_hip, table, V, b, rated, K, user_idx)
    print(case_id(p), report['form'], report['id_bits'], report['image'], report['blocks'], report['pieces'], report['flagged'])
    assert_same_as_fp32_and_oracle(refine, fp32, U, V, b, rated, K)
    assert all(case['victim'] in refine[0][r] for r in range(len(U)))
    users = 128 if id_bits == 16 else 192
    assert (report['form'], report['id_bits'], report['image']) == (form, id_bits, image), report
    assert report['blocks'] == (len(U) + users - 1) // users and report['flagged'] == 0 and not any(report['flags']), report
    if same_range:
        n_tiles = (len(V) + 31) // 32
        assert report['pieces'] % report['blocks'] == 0
        tps = -(-n_tiles // (report['pieces'] // report['blocks']))
        assert tps >= 2 and p['first_tile'] // tps == (p['first_tile'] + 1) // tps, (report, tps)
    return report
