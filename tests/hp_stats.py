"""Truth, plain restatement and rounding-count bounds for the running statistics and the device error estimator
--  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Inputs are exact: the fp64 lift matrix L [n][p], the sizes of its MERGE GROUPS (the samples whose moments are taken about
one running mean and merged by one Chan step: a chunk collected with accumulate = 2, or everything collected with
accumulate = 1 between two merges) and, for the estimator, the fp64 normals Xi [1024][n].

    truth      two-pass mean and biased covariance, draws = Xi (L - 1 mean^T) / sqrt(n (n - 1)) and their 0.95-quantiles,
               all in numpy.longdouble (validated against mpmath in tests/test_hp_stats_host.py)
    plain      the engine's own route in fp64 NumPy: group by group the moments about the running mean (zero before the
               first group), the Chan merge with the kernels' coef = n nb / (n + nb) - nb and wgt = 1 / (n + nb),
               D += Xi L and s += Xi 1 chunk by chunk.  Carries the three CPU mutations (MUTATIONS).
    bound      what round-off may do to a correct fp64 implementation of that route, evaluated in long double from the
               truth.  Every term is  u x (roundings on the path) x (magnitudes summed),  u = 2^-53.

Where the constants of the bound come from (csrc/k_lift.hip, csrc/k_error.hip).  A sum of N terms has at most N - 1
additions on the path of any term WHATEVER the order -- four waves' partial sums met in LDS, 16-sample steps, slices added
in order, two accumulate = 1 launches added in the pending buffer are all trees over the group's samples (added zeros are
exact) -- so the order never enters, only N.

  Q_ab = sum_s d_sa d_sb,  d = fl(l - m):  two subtractions, one product (the matrix instruction fuses the addition), at
      most count - 1 additions:           (count + 2) u sum_s |d_sa| |d_sb|
  S_a = sum_s d_sa:                       E_S = count u sum_s |d_sa|
  T_ab = coef (S_a inv)(S_b inv):  coef = fl(fl(n nb / (n + nb)) - nb) is off by u (w + |coef|) <= 2 u nb  (w = n nb / (n +
      nb) <= nb: the cancellation in w - nb when n >> nb is counted here); inv = fl(1 / nb) enters twice, two products
      with it, the product of the two, the product with coef: 6 roundings, 7 taken:
                                          (2 u nb + 7 u |coef|) |delta_a| |delta_b| + |coef| (E_Sa |delta_b| + |delta_a| E_Sb) / nb
  the running mean the group was taken about is itself off by at most Em: Q - nb delta delta^T does not depend on the
      shift, the w delta delta^T term does:     w (|delta_a| Em_b + Em_a |delta_b|)
  the merge, M2 + (Q + T): two additions:  u |Q + T| + u |M2_new|     (the "number of merges x u x |M2|" term)
  cov = M2 * fl(1 / n):                    2 u |cov|
  mean_new = m + S * fl(1 / (n + nb)):     Em_new = Em n / (n + nb) + (E_S + 2 u |S|) / (n + nb) + u |mean_new|
      (an error e of m goes into S as -nb e: e n / (n + nb) is left of it)
  D_da = sum_k xi_dk l_ka over all N samples so far (a tree again, fused products):   E_D = N u sum_k |xi_dk| |l_ka|
  s_d = sum_k xi_dk:                       E_s = N u sum_k |xi_dk|
  x_da = fma(-s_d, mean_a, D_da) * scale:  core = D - s mean is off by E_D + E_s |mean_a| + |s_d| Em_a + u |core| (this is
      the D - s mean cancellation: E_D is of the size of D, not of core); scale = 1 / sqrt(nt (nt - 1)) two roundings,
      the product one:                    E_x = E_core scale + 3 u |x|
  a quantile of 1024 values moves by at most the largest move of a value (order statistics are 1-Lipschitz in the
      maximum norm); the interpolation is three roundings:   E_q = max_d E_x + 3 u q
  ||x_d||_2 over p features: p fused products and additions, the square root:   ||E_x[d]||_2 + (p + 2) u ||x_d||
All of it first order in u; the factor 1 + 2^-10 on every bound covers the higher orders (N u < 3e-13 here)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -10
ND = 1024
MUTATIONS = ("drop", "coef", "stale")


class Reference:
    """Truth and bounds of the statistics after the last group (mean, cov, Em, Ecov) and after every group (snaps: n,
    mean, Em), from one pass over the groups in long double."""

    def __init__(self, L, groups):
        Lq = np.asarray(L, dtype=LD)
        N, p = Lq.shape
        groups = [int(c) for c in groups if c > 0]
        assert sum(groups) == N
        self.n = N
        self.mean = Lq.sum(0) / N
        dc = Lq - self.mean
        self.cov = dc.T @ dc / N
        n, i = 0, 0
        m = np.zeros(p, dtype=LD)
        M2 = np.zeros((p, p), dtype=LD)
        Em = np.zeros(p, dtype=LD)
        EM2 = np.zeros((p, p), dtype=LD)
        self.snaps = []
        for cnt in groups:
            d = Lq[i:i + cnt] - m
            ad = np.abs(d)
            nb = LD(cnt)
            w = n * nb / (n + nb)
            coef = w - nb
            S = d.sum(0)
            delta = S / nb
            adl = np.abs(delta)
            ES = cnt * U * ad.sum(0)
            QT = d.T @ d + coef * np.outer(delta, delta)
            M2 = M2 + QT
            EM2 += ((cnt + 2) * U * (ad.T @ ad)
                    + (2 * U * nb + 7 * U * abs(coef)) * np.outer(adl, adl)
                    + abs(coef) * (np.outer(ES, adl) + np.outer(adl, ES)) / nb
                    + w * (np.outer(adl, Em) + np.outer(Em, adl))
                    + U * np.abs(QT) + U * np.abs(M2))
            m_new = m + S / (n + nb)
            Em = Em * n / (n + nb) + (ES + 2 * U * np.abs(S)) / (n + nb) + U * np.abs(m_new)
            m, n, i = m_new, n + cnt, i + cnt
            self.snaps.append((n, m, Em * SLACK))
        self.chan_cov = M2 / N          # the route in exact arithmetic: equals cov (host test)
        self.Em = Em * SLACK
        self.Ecov = (EM2 / N + 2 * U * np.abs(self.cov)) * SLACK


def plain_stats(L, groups, mutate=None):
    """The engine's route in fp64 NumPy; returns n, mean, cov and the (n, mean) after every group.  mutate: one of
    MUTATIONS -- 'drop': the last sample of the LARGEST group (the first of them) is left out of its moments, the group
    still counts it -- what a wave's quarter one step short does to a chunk of more than 16 samples;
    'coef': coef = n nb / (n + nb) without the - nb; 'stale': a group's moments are taken about the mean as it stood
    before the PREVIOUS group, and the mean is advanced from the current one."""
    L = np.asarray(L, dtype=np.float64)
    groups = [int(c) for c in groups if c > 0]
    p = L.shape[1]
    n, i = 0.0, 0
    mean, prev = np.zeros(p), np.zeros(p)
    M2 = np.zeros((p, p))
    snaps = []
    for k, cnt in enumerate(groups):
        X = L[i:i + cnt]
        if mutate == "drop" and k == int(np.argmax(groups)):
            X = X[:-1]
        d = X - (prev if mutate == "stale" else mean)
        Q, S = d.T @ d, d.sum(0)
        nb = float(cnt)
        coef = n * nb / (n + nb) - (0.0 if mutate == "coef" else nb)
        inv = 1.0 / nb
        M2 = M2 + (Q + coef * np.outer(S * inv, S * inv))
        prev = mean
        mean = mean + S * (1.0 / (n + nb))
        n, i = n + nb, i + cnt
        snaps.append((int(n), mean.copy()))
    return int(n), mean, M2 * (1.0 / n), snaps


def quantile95(v, axis=0):
    """numpy.quantile(v, 0.95, method='linear') in v's own precision: the position 0.95 (len - 1) and its fractional part
    are numpy's (and the kernel's) fp64 numbers -- they define the quantile --, the interpolation is v's arithmetic
    (numpy.quantile itself is not trusted to keep long double throughout; the host test compares the two)."""
    v = np.sort(np.asarray(v), axis=axis)
    v = np.moveaxis(v, axis, 0)
    pos = 0.95 * (v.shape[0] - 1)
    lo = int(np.floor(pos))
    t = v.dtype.type(pos - lo)
    return v[lo] + (v[lo + 1] - v[lo]) * t


class EstReference:
    """Truth and bounds of the running estimator after every chunk that has a check.  chunks: sizes of the estimator's
    chunks (one acc launch each), in order; Xi [1024][N] the normals of the samples in that order; ref: the Reference of
    the statistics, whose snapshots the checks read (check_groups[c] = index of the merge group after which chunk c's
    check runs, or None for no check)."""

    def __init__(self, L, Xi, chunks, ref, check_groups):
        Lq, Xq = np.asarray(L, dtype=LD), np.asarray(Xi, dtype=LD)
        p = Lq.shape[1]
        D = np.zeros((ND, p), dtype=LD)
        AD = np.zeros((ND, p), dtype=LD)
        s = np.zeros(ND, dtype=LD)
        As = np.zeros(ND, dtype=LD)
        i = 0
        self.checks = {}
        for c, cnt in enumerate(chunks):
            if cnt > 0:
                Xc, Lc = Xq[:, i:i + cnt], Lq[i:i + cnt]
                D, AD = D + Xc @ Lc, AD + np.abs(Xc) @ np.abs(Lc)
                s, As = s + Xc.sum(1), As + np.abs(Xc).sum(1)
                i += cnt
            if check_groups[c] is None:
                continue
            n, mean, Em = ref.snaps[check_groups[c]]
            assert n == i, (n, i)
            scale = 1 / np.sqrt(LD(n) * (n - 1))
            core = D - np.outer(s, mean)
            x = core * scale
            ED, Es = n * U * AD, n * U * As
            Ecore = ED + np.outer(Es, np.abs(mean)) + np.outer(np.abs(s), Em) + U * np.abs(core)
            Ex = (Ecore * scale + 3 * U * np.abs(x)) * SLACK
            feat = quantile95(np.abs(x))
            norms = np.sqrt((x * x).sum(1))
            tot = quantile95(norms)
            Enorm = np.sqrt((Ex * Ex).sum(1)) + (p + 2) * U * norms
            self.checks[c] = dict(n=n, mean=mean, Em=Em, x=x, feat=feat, tot=tot,
                                  Efeat=(Ex.max(0) + 3 * U * feat) * SLACK, Etot=(Enorm.max() + 3 * U * tot) * SLACK)
        self.D, self.s = D, s
        self.ED, self.Es = i * U * AD * SLACK, i * U * As * SLACK


def plain_estimator(L, Xi, chunks, snaps, check_groups):
    """fp64 NumPy: D += Xi_c L_c, s += Xi_c 1 chunk by chunk; a check is x = (D - s mean^T) * scale with the plain
    statistics' mean after its group, and the two quantiles.  Returns D, s, {chunk: (feat, tot)}."""
    L, Xi = np.asarray(L, dtype=np.float64), np.asarray(Xi, dtype=np.float64)
    D, s, i, out = np.zeros((ND, L.shape[1])), np.zeros(ND), 0, {}
    for c, cnt in enumerate(chunks):
        if cnt > 0:
            D = D + Xi[:, i:i + cnt] @ L[i:i + cnt]
            s = s + Xi[:, i:i + cnt].sum(1)
            i += cnt
        if check_groups[c] is not None:
            n, mean = snaps[check_groups[c]]
            x = (D - np.outer(s, mean)) * (1.0 / np.sqrt(n * (n - 1.0)))
            out[c] = (quantile95(np.abs(x)), quantile95(np.linalg.norm(x, axis=1)))
    return D, s, out


def ratio(err, bound):
    """max of err / bound over the entries, 0 / 0 counting as 0 and x / 0 as inf."""
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


# ---- input families (seeded; nothing on disk) -----------------------------------------------------------------------------
def scaling_exponents(p, seed):
    return np.random.default_rng(seed + 77).integers(-40, 41, size=p)


def family(name, n, p, seed):
    """'gauss': centred, sigma 1.  'liftlike': positive entries around 1 / p, every row summing to 0.8 (to round-off):
    singular covariance.  'offset4' / 'offset6': mean 1, sigma 1e-4 / 1e-6.  'scaled': 'gauss' with column a times
    2^k(a), |k| <= 40.  'degenerate': 'gauss' with column 0 zero, column 1 the constant 0.37, column 3 = column 2 and
    column 5 = -column 4 (as far as p reaches)."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, p))
    if name == "gauss":
        return G
    if name == "liftlike":
        B = (1.0 + 0.5 * np.tanh(G)) / p
        return 0.8 * B / B.sum(1, keepdims=True)
    if name in ("offset4", "offset6"):
        return 1.0 + (1e-4 if name == "offset4" else 1e-6) * G
    if name == "scaled":
        return G * np.exp2(scaling_exponents(p, seed))
    if name == "degenerate":
        G[:, 0] = 0.0
        if p > 1:
            G[:, 1] = 0.37
        if p > 3:
            G[:, 3] = G[:, 2]
        if p > 5:
            G[:, 5] = -G[:, 4]
        return G
    raise ValueError(name)


# ---- the GPU cases (tests/test_gpu_stats_accuracy.py runs them, tests/test_hp_stats_host.py vets them on the CPU) ------
# A plan is a list of steps on ONE injected batch, front to back:
#   ("acc1", count)  collect into the pending buffer        ("merge",)  lsspa_stats_merge
#   ("acc2", count)  collect and merge at once              ("chunks", chunk, n_chunks)  lsspa_lift_collect_chunks
#   ("group", counts)  lsspa_group_collect, a check after every chunk that has samples
def plan_groups(plan):
    """The merge groups of a plan."""
    groups, pend = [], 0
    for st in plan:
        if st[0] == "acc1":
            pend += st[1]
        elif st[0] == "merge":
            groups.append(pend)
            pend = 0
        elif st[0] == "acc2":
            groups.append(st[1])
        elif st[0] == "chunks":
            groups += [st[1]] * st[2]
        elif st[0] == "group":
            groups += [c for c in st[1] if c > 0]
    assert pend == 0, "a plan ends merged"
    return groups


def each(kind, counts):
    out = []
    for c in counts:
        out += [("acc1", c), ("merge",)] if kind == "acc1" else [("acc2", c)]
    return out


SMALL_COUNTS = {1: (1, 512, 3), 15: (15, 16, 511), 16: (17, 63, 1), 17: (64, 65, 1), 127: (512, 3, 17),
                128: (511, 16, 65, 1)}
GENERAL = ("gauss", "liftlike", "offset4", "offset6")

# (name, p, plan, families)
STATS_CASES = []
for _p, _c in SMALL_COUNTS.items():
    _fam = GENERAL + (("scaled", "degenerate") if _p in (17, 128) else ())
    if _p == 1:         # one column that sums to a constant IS a constant: blind to every mutation (host test), left out
        _fam = tuple(f for f in _fam if f != "liftlike")
    STATS_CASES.append((f"small_merge_p{_p}", _p, each("acc1", _c), _fam))
    STATS_CASES.append((f"small_fused_p{_p}", _p, each("acc2", _c), _fam))
STATS_CASES += [
    ("small_fused_p16_n_much_larger_than_nb", 16, each("acc2", (512,) + (1,) * 40), GENERAL),
    ("multi_p7_32x1", 7, [("chunks", 1, 32)], GENERAL + ("degenerate",)),
    ("multi_p16_2x512", 16, [("chunks", 512, 2)], GENERAL + ("scaled",)),
    ("multi_p100_32x1_after_lead", 100, [("acc2", 9), ("chunks", 1, 32)], GENERAL),
    ("multi_p128_2x512", 128, [("chunks", 512, 2)], GENERAL),
    ("batch_p129", 129, each("acc1", (1, 17, 100)), GENERAL + ("scaled", "degenerate")),
    ("batch_p192", 192, each("acc2", (17, 100, 1)), GENERAL),
    ("batch_p257", 257, each("acc1", (100, 1, 17)), GENERAL),
    ("sliced_p130_twice", 130, [("acc1", 128), ("acc1", 128), ("merge",), ("acc2", 128)], GENERAL + ("scaled", "degenerate")),
    ("sliced_p100_last_slice_short", 100, [("acc1", 513), ("acc1", 600), ("merge",), ("acc2", 513), ("acc2", 600)],
     GENERAL + ("scaled",)),
    ("sliced_p257_twice", 257, [("acc1", 1300), ("acc1", 9), ("merge",), ("acc2", 17)], ("gauss", "offset4")),
    ("sliced_p257_at_once", 257, [("acc2", 9), ("acc2", 1300)], ("gauss", "offset6")),
    ("sliced_p300_twice", 300, [("acc2", 9), ("acc1", 2000), ("acc1", 1), ("merge",)], ("gauss", "liftlike")),
    ("sliced_p300_at_once", 300, [("acc2", 9), ("acc2", 2000)], ("offset4",)),
    ("merge2_p257", 257, each("acc1", (9, 200, 1300)), ("gauss", "offset4", "scaled")),
    ("merge2_p300", 300, each("acc1", (9, 200, 1300)), ("liftlike", "offset6")),
]
# the sliced cases' (samples, p) -> the samples per slice they were chosen for (asserted against the library's own rule,
# lsspa_debug_stats_slices)
SLICE_EDGES = {(128, 130): [64, 64], (513, 100): [64] * 8 + [1], (600, 100): [64] * 9 + [24],
               (1300, 257): [80] * 16 + [20] + [0] * 3, (2000, 300): [112] * 17 + [96] + [0] * 2}


EST_COUNTS = (15, 1, 16, 17, 64, 200)       # (no check at n = 1: its scale is 1 / 0)
# (name, p, how, counts, stride, families): how = 'check' (collect accumulate = 2, advance, check_enqueue), 'draws' (...,
# running_draws, quantiles_enqueue), 'group' (one lsspa_group_collect), 'group0' (the same with an empty chunk: the
# chunk-by-chunk form of that call), 'thin' (history + lsspa_error_draws with host normals + lsspa_error_quantiles)
EST_CASES = [
    ("est_check_p12", 12, "check", EST_COUNTS, 1, GENERAL + ("scaled", "degenerate", "ties1", "ties2")),
    ("est_draws_p128", 128, "draws", EST_COUNTS, 3, GENERAL + ("scaled",)),
    ("est_check_p129", 129, "check", EST_COUNTS, 1, ("gauss", "offset4", "degenerate")),
    ("est_draws_p300", 300, "draws", EST_COUNTS, 3, ("gauss", "liftlike")),
    ("est_group_p12", 12, "group", EST_COUNTS, 3, GENERAL + ("scaled", "degenerate", "ties1", "ties2")),
    ("est_group_p128", 128, "group", EST_COUNTS, 1, GENERAL),
    ("est_group_p100_inside_batch", 100, "group", (9, 5, 16, 1, 33, 17), 1, GENERAL + ("scaled",)),
    ("est_group_p100_empty_chunk", 100, "group0", (9, 5, 0, 16, 1, 33, 17), 3, ("gauss", "offset4")),
    ("est_thin_p128", 128, "thin", (17, 64), 1, ("gauss", "offset4")),
    ("est_thin_p129", 129, "thin", (17, 64), 1, ("gauss", "liftlike")),
]


def est_family(name, n, p, seed):
    """The families above and 'ties1' / 'ties2': one non-zero sample, and two samples with opposite entries (the mean is
    exactly zero), the rest zero.  The draws of a feature are then one or two of the device's normals times a constant --
    1024 values of one shape, but NOT equal ones (the normals differ): equal neighbours need repeated normals, which
    only the thin form with the caller's normals can give (lerp_inputs below)."""
    if name == "ties1":
        L = np.zeros((n, p))
        L[n // 2] = np.random.default_rng(seed).standard_normal(p)
        return L
    if name == "ties2":
        L = np.zeros((n, p))
        v = np.random.default_rng(seed).standard_normal(p)
        L[1], L[n - 2] = v, -v
        return L
    return family(name, n, p, seed)


def case_seed(name, fam):
    return sum(ord(ch) * (k + 1) for k, ch in enumerate(name + "/" + fam)) % 100003


def est_layout(how, counts):
    """plan, estimator chunks and check_groups of an estimator case.  A 'group' case whose counts start with 9 takes those
    9 samples by themselves first (accumulate = 2 + advance, no check): statistics are there already and the group
    starts inside the batch."""
    counts = list(counts)
    if how in ("check", "draws"):
        return each("acc2", counts), counts, list(range(len(counts)))
    if how == "thin":
        return each("acc2", counts), [sum(counts)], [len(counts) - 1]
    lead = counts[:1] if counts[0] == 9 else []
    rest = counts[len(lead):]
    plan = each("acc2", lead) + [("group", rest)]
    cg, g = [], len(lead) - 1
    for c in rest:
        g += 1 if c > 0 else 0
        cg.append(g if c > 0 else None)
    return plan, lead + rest, [None] * len(lead) + cg


# ---- the interpolation of the quantile, to the bit ----------------------------------------------------------------------
# An err <= bound assertion cannot tell numpy's _lerp (from b's side when t >= 0.5) from the a-side form everywhere: the
# two differ by one rounding.  Bitwise they can be told apart where b - a is not exact, i.e. where the two neighbours are
# more than a factor two apart.  The thin form takes the caller's normals, so the 1024 |draws| of a feature can be made
# to take two values, 972 times v and 52 times about 1001 v (v's low bits are lost in b - a): the 0.95-quantile (position 971.85) then sits between them.
LERP_N = 4


def lerp_inputs(p, seed, n_small=972):
    """Integer lift vectors [4][p] (their mean is exact) and integer normals [1024][4] = w_d * (2, -1, 0, 0), w_d = +-1 for
    n_small draws and +-1001 for the rest: core = Xi L - rowsum(Xi) mean = w_d (2 l_0 - l_1 - mean) is exact, a draw is ONE
    rounding (the product with the scale).  Returns L, Xi."""
    rng = np.random.default_rng(seed)
    L = rng.integers(-40, 41, size=(LERP_N, p)).astype(np.float64)
    L[0] += 100.0           # 2 l_0 - l_1 - mean != 0
    w = np.where(np.arange(ND) < n_small, 1.0, 1001.0) * rng.choice([-1.0, 1.0], size=ND)
    Xi = np.outer(rng.permutation(w), [2.0, -1.0, 0.0, 0.0])
    return L, Xi


def lerp_candidates(va, vb):
    """The values a correct b-side interpolation may give and those the a-side form may give between neighbours va <= vb:
    as numpy evaluates it (t = 0.95 * 1023 - 971, the product and the sum each rounded) or as a compiler that fuses
    multiply-adds does (t, and the product with the sum, in one rounding each; what hipcc's default contraction makes of
    quantile_body).  Exact rational arithmetic, rounded to nearest."""
    from fractions import Fraction as Fr
    d = vb - va
    t = 0.95 * (ND - 1) - 971.0
    tf = float(Fr(0.95) * (ND - 1) - 971)
    b_side = {vb - d * (1.0 - t), float(Fr(vb) - Fr(d) * Fr(1.0 - tf))}
    a_side = {va + d * t, float(Fr(va) + Fr(d) * Fr(tf))}
    return b_side, a_side
