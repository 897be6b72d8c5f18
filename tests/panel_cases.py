"""The cases of the truth tests of the per-ordering general path (gather -> chol_diag2 -> chol_panel2 with X tiles and
fused lift scan -> strip2 -> lift; csrc/k_factor.hip, csrc/k_lift.hip), their data and their orderings.  Importable
without a GPU: tests/test_panel_plan_host.py checks on the CPU, through the library's own launch rule
(lsspa_debug_panel_plan: panel_plan of csrc/k_factor.hip under run_slice's shape rules), that the list reaches every
class it was written for; tests/test_gpu_panel_edges.py runs it.

What a panel launch decides (launch_chol2_panel) and where a case has to sit to see the decision:

    p_pad = round_up(p + 1, 128), n_panel = p_pad / 128 - 1 launches with L tiles (+ one, X tiles only, in tri mode
        without developer flag 128): the panel-count edges are p = 127 | 128, 255 | 256, 383 | 384, 511 | 512
    p_live = round_up(p + 1, 16): all-zero tiles at or beyond it are skipped; xlast = (no L tiles and
        p_live <= p_pad - 16) takes another instantiation of the kernel
    grouped = (n_mats % 8 == 0 and n_lt > 1): another workgroup -> (matrix, tile) map; n_lt > 1 needs p_pad >= 384
    fp64 | fp32, tri | rect, and in tri mode the three forms of the lift (fused scan, flag 512, flag 128)

Data: hp_ref.gen(p, n, m, 1.0, seed) with n = 2 p + 40 and, in tri mode, m = p + 50; the seed depends on (p, m) alone,
so that the cases of one shape -- precisions, flags, batch sizes -- share one long-double truth."""
from collections import namedtuple

import numpy as np

F64, F32 = "float64", "float32"
Case = namedtuple("Case", "name p n m dtype flags B anti cls")

SMALL_P_MAX = 127           # p + 1 <= 128: fp64 tri mode takes the fused kernel unless developer flag 1024 is set
N_ORDERS = 16               # orderings_of(p, B) is a prefix of one sequence of this many per p

PANEL_COUNT_P = (127, 128, 255, 256, 257, 383, 384, 385, 511, 512)
XLAST_ON_P = (239, 367, 495)        # p_live = p_pad - 16: exactly one dead 16-column block
XLAST_OFF_P = (240, 368, 496)       # p_live = p_pad
ONE_LIVE_P = (256, 384)             # one live 16-row block in the last panel (p_live = p_pad - 112)
P_LIVE_P = (271, 272, 143, 144)     # p + 1 = 0 and 1 (mod 16) inside a panel
FP32_SMALL_P = (15, 16, 63, 64, 65, 111, 112, 127)
RECT_M_EDGES = (1, 15, 16, 17, 127, 128, 129)       # col_live = round_up(m, 16), m_pad = round_up(m, 128)
DISPATCH_P = 300            # p_pad = 384: launch 0 has two L tiles a matrix (grouped possible), p_live = 304
DISPATCH_P512 = 385         # p_pad = 512: launches with 3, 2, 1 and 0 L tiles
RECT_M = 100


def tri_m(p):
    return p + 50


def n_of(p):
    return 2 * p + 40


def seed_of(p, m):
    return 9000 + 7 * p + m % 1000


def flags_for(p, dtype, tri, flags):
    """Developer flag 1024 (general path also for small problems) where the fused small-p kernel would run."""
    return flags | (1024 if (tri and dtype == F64 and p <= SMALL_P_MAX) else 0)


def _case(cls, p, dtype, B, anti, m=None, flags=0):
    tri = m is None
    m = tri_m(p) if tri else m
    flags = flags_for(p, dtype, tri, flags)
    name = f"{cls}_{'tri' if tri else f'rect{m}'}_p{p}_{dtype}_f{flags}_B{B}{'a' if anti else ''}"
    return Case(name, p, n_of(p), m, dtype, flags, B, anti, cls)


def _cases():
    out = []
    both = (F64, F32)
    # panel-count edges; p = 127 in tri mode runs the lone X-only launch (n_panel = 0)
    for p in PANEL_COUNT_P:
        for dt in both:
            out.append(_case("panel_count", p, dt, 3, True))
    for p in (255, 256, 257, 383, 385):
        out.append(_case("panel_count", p, F64, 3, True, m=RECT_M))
    for p in (257, 385):
        out.append(_case("panel_count", p, F32, 3, True, m=RECT_M))
    # xlast on / off, one live block
    for cls, ps in (("xlast_on", XLAST_ON_P), ("xlast_off", XLAST_OFF_P), ("one_live_block", ONE_LIVE_P)):
        for p in ps:
            for dt in both:
                out.append(_case(cls, p, dt, 3, True))
    for p in XLAST_ON_P[:2]:
        out.append(_case("xlast_on", p, F64, 3, True, flags=512))       # the X-only launch without the fused scan
    # p_live inside a panel: the panel kernel's row_live (tri) and the strip kernel's (rect)
    for p in P_LIVE_P:
        for dt in both:
            out.append(_case("p_live", p, dt, 3, True))
        out.append(_case("p_live", p, F64, 3, True, m=RECT_M))
    # the three forms of the lift in tri mode (flags 0 are the panel_count cases of the same p)
    for p in (127, 257, 385):
        for dt in both:
            for flags in (512, 128):
                out.append(_case("mode", p, dt, 3, True, flags=flags))
    # fp32 below one panel: fp64 takes the fused kernel there and hides the general path
    for p in FP32_SMALL_P:
        out.append(_case("fp32_small", p, F32, 3, True))
    # dispatch, tri: n_mats = 2 B (x 2 antithetical)
    for dt in both:
        out.append(_case("n_mats_2", DISPATCH_P, dt, 1, False))
        out.append(_case("odd_count", DISPATCH_P, dt, 3, False))            # 3 orderings, 6 matrices
        out.append(_case("grouped_8", DISPATCH_P, dt, 2, True))
        out.append(_case("grouped_8", DISPATCH_P, dt, 4, False))            # the unpaired gather under the grouped map
        out.append(_case("ungrouped_partner", DISPATCH_P, dt, 3, True))     # 12
        out.append(_case("grouped_16", DISPATCH_P, dt, 4, True))
        out.append(_case("ungrouped_partner", DISPATCH_P, dt, 5, True))     # 20
        out.append(_case("grouped_24", DISPATCH_P, dt, 6, True))
        out.append(_case("grouped_p512", DISPATCH_P512, dt, 2, True))       # n_lt = 3, 2 grouped; 1, 0 not
        out.append(_case("ungrouped_partner", DISPATCH_P512, dt, 1, True))  # 4 (B = 3: the panel_count case of p = 385)
    # dispatch, rect: n_mats = B (x 2 antithetical)
    out.append(_case("n_mats_1", DISPATCH_P, F64, 1, False, m=RECT_M))
    out.append(_case("odd_count", DISPATCH_P, F64, 5, False, m=RECT_M))
    for dt in both:
        out.append(_case("grouped_8", DISPATCH_P, dt, 8, False, m=RECT_M))
        out.append(_case("grouped_8", DISPATCH_P, dt, 4, True, m=RECT_M))
        out.append(_case("ungrouped_partner", DISPATCH_P, dt, 7, False, m=RECT_M))
        out.append(_case("ungrouped_partner", DISPATCH_P, dt, 3, True, m=RECT_M))
        out.append(_case("grouped_16", DISPATCH_P, dt, 16, False, m=RECT_M))
        out.append(_case("ungrouped_partner", DISPATCH_P, dt, 15, False, m=RECT_M))
        out.append(_case("grouped_24", DISPATCH_P, dt, 12, True, m=RECT_M))
        out.append(_case("ungrouped_partner", DISPATCH_P, dt, 11, True, m=RECT_M))
        out.append(_case("grouped_p512", DISPATCH_P512, dt, 8, False, m=RECT_M))
        out.append(_case("ungrouped_partner", DISPATCH_P512, dt, 7, False, m=RECT_M))
    # rect: the strip kernel's col_live and the last strip's width
    for m in RECT_M_EDGES:
        for dt in both:
            out.append(_case("rect_col_live", 130, dt, 3, True, m=m))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}

# test b (factors against the truth): panel-count and xlast edges, both precisions
FACTOR_P = tuple(sorted(set(PANEL_COUNT_P + XLAST_ON_P + XLAST_OFF_P)))
# test c (composition) and d (workspace history)
COMPOSITION_P = (257, 385)


def is_tri(c):
    return c.m >= c.p


def n_ord_of(c):
    return c.B * (2 if c.anti else 1)


def data_of(p, n, m):
    import hp_ref
    return hp_ref.gen(p, n, m, 1.0, seed_of(p, m))


def orderings_of(p, B):
    """The identity, its reverse and seeded random orderings, B of them: a prefix of one sequence per p."""
    assert 1 <= B <= N_ORDERS
    rng = np.random.default_rng(p)
    rows = [np.arange(p), np.arange(p)[::-1]] + [rng.permutation(p) for _ in range(N_ORDERS - 2)]
    return np.ascontiguousarray(np.array(rows[:B], dtype=np.int32))
