"""Which cloud sizes sit on a boundary of a GICP kernel's grid -- found by QUERYING a plan, never from a copy of the kernels'
constants (the sibling of tests/eval_plan_sizes.py for the GICP row).  `plan` is any callable n -> mapping with the fields of
gicp_diag_plan (plan of a GeneralizedIterativeClosestPoint handle, or a stub with known break points:
tests/test_gicp_plan_sizes.py).

A boundary b is the FIRST size of a new grid value: plan(b - 1) and plan(b) differ in that field.  Every boundary is
probed at b - 1, b and b + 1.  A grid never shrinks as the cloud grows, so a boundary is found by bisection (a plan of a
million sizes costs twenty queries, not a million); is_boundary is the check every test makes before it relies on one."""

FIELDS = ("knn_blocks", "correspond_blocks", "functor_blocks", "server_blocks")
# grid sizes whose first occurrence is probed: one block, two, the eight shard counters of the objective server and
# either side of them (7, 8, 9), and the second round of the deal (16, 17)
BLOCK_COUNTS = (1, 2, 7, 8, 9, 16, 17)


def first_reaching(plan, field, blocks, hi):
    """Smallest n in [1, hi] whose grid has at least `blocks` blocks, or None if plan(hi) has fewer."""
    if plan(hi)[field] < blocks:
        return None
    lo, up = 1, hi  # invariant: plan(up) >= blocks; everything below lo has fewer
    while lo < up:
        mid = (lo + up) // 2
        if plan(mid)[field] >= blocks:
            up = mid
        else:
            lo = mid + 1
    return lo


def is_boundary(plan, field, b):
    """plan changes at b in `field` (b = 1, the smallest cloud, counts as the first size of the one-block grid)."""
    return b == 1 or plan(b - 1)[field] != plan(b)[field]


def block_boundaries(plan, field, hi, counts=BLOCK_COUNTS):
    """dict blocks -> first size whose grid has exactly that many blocks, for every count the plan takes on in [1, hi - 1]
    (so that b + 1 <= hi); a count the plan jumps over or never reaches is not reported."""
    out = {}
    for c in counts:
        b = first_reaching(plan, field, c, hi)
        if b is not None and b <= hi - 1 and plan(b)[field] == c:
            out[c] = b
    return out


def cap_boundary(plan, field, hi):
    """(b, period): b = the first size at which the grid has its final value plan(hi), period = how many sizes the value
    before it held.  From b on the grid stays put; it covers one more period in one pass, so b + period is the first size
    at which a thread of the capped grid walks a second point (the grid-strided regime).  None unless the final value then
    holds for more than two periods within [1, hi] -- a cap, not the end of the range -- or if the grid never changes."""
    top = plan(hi)[field]
    b = first_reaching(plan, field, top, hi)
    if b is None or b == 1:
        return None
    prev = first_reaching(plan, field, plan(b - 1)[field], hi)
    period = b - prev
    if hi - b <= 2 * period:
        return None
    return b, period


def around(sizes):
    """Sorted, de-duplicated b - 1, b, b + 1 of every size given (sizes below 1 dropped)."""
    s = set()
    for b in sizes:
        s.update((b - 1, b, b + 1))
    return sorted(x for x in s if x >= 1)


def functor_sweep_sizes(plan, hi, counts=BLOCK_COUNTS):
    """Source sizes of the functor sweep: for the functor kernel's and the server's grid, the first size of each block count
    of `counts` and the sizes either side of it."""
    s = []
    for field in ("functor_blocks", "server_blocks"):
        s += list(block_boundaries(plan, field, hi, counts).values())
    return around(s)


def cap_sizes(plan, field, hi):
    """[b - 1, b, b + 1, b + period, b + period + 1] of the field's cap (the boundary +- 1, then one period beyond it: the
    last size one pass covers is b + period - 1, so b + period and its successor are the first two strided ones), or []
    if the plan has no cap below hi."""
    c = cap_boundary(plan, field, hi)
    if c is None:
        return []
    b, period = c
    return [b - 1, b, b + 1, b + period, b + period + 1]
