"""Which source sizes sit on a boundary of an evaluation kernel's block plan -- found by QUERYING a plan, never from a
copy of its formulae.  `plan` is any callable n -> mapping with the fields of ndt_diag_eval_plan (evalPlan of a handle, or
a stub with known break points: tests/test_eval_plan_sizes.py).

A boundary b is the FIRST size of a new regime: plan(b - 1) and plan(b) differ in the respect the boundary is named for.
Every boundary is probed at b - 1, b and b + 1."""
import numpy as np

FIELDS = ("ppb", "fused_blocks", "launch_blocks", "server_blocks", "batch_blocks")
# sizes probed whatever the plan says: the smallest scans, the 64-lane edge, and one size that is no multiple of 8
SMALL_SIZES = (1, 2, 7, 63, 64, 65, 1003)
# every boundary the chooser knows (a plan that never reaches one within `hi` simply does not report it)
EVAL_BOUNDARIES = ("ppb_leaves_min", "ppb_saturates",
                   "fused_two_blocks", "fused_max", "fused_cap", "fused_strided",
                   "launch_two_blocks", "launch_max", "launch_cap", "launch_strided",
                   "server_two_blocks", "server_max", "server_cap", "server_walk")
BATCH_BOUNDARIES = ("batch_2_blocks", "batch_3_blocks", "batch_9_blocks")  # 8 -> 9: the modulus of the XCD deal


def plan_table(plan, hi):
    """(hi + 1, 5) int array: row n = plan(n) in FIELDS order (row 0 is not used by the chooser)."""
    t = np.zeros((hi + 1, len(FIELDS)), dtype=np.int64)
    for n in range(hi + 1):
        p = plan(n)
        t[n] = [p[f] for f in FIELDS]
    return t


def _changes(col):
    """Sizes n >= 2 with col[n] != col[n - 1]."""
    return (np.nonzero(col[2:] != col[1:-1])[0] + 2).tolist()


def _first(mask):
    """First n >= 1 with mask[n], or None."""
    idx = np.nonzero(mask[1:])[0]
    return int(idx[0]) + 1 if len(idx) else None


def boundaries(plan, hi, table=None):
    """dict name -> b for every boundary of EVAL_BOUNDARIES + BATCH_BOUNDARIES the plan reaches in [2, hi - 1] (so that
    b + 1 <= hi).  What the names mean:
      ppb_leaves_min / ppb_saturates   first / last size at which points-per-block changes (the last one only if ppb then
                                       stays put for as long as its previous value held at least)
      X_two_blocks                     the grid of form X goes from one block to two
      X_max                            the grid first reaches the largest value it has in [1, hi]
      X_cap                            the last size at which the grid changes, given that it then stays put for longer than
                                       its previous value held (a cap, not the end of the range)
      fused_strided / server_walk      first size that blocks x ppb no longer covers in one pass
      launch_strided                   launch_cap + the length the previous grid value held (its blocks have no ppb: the
                                       capped grid covers exactly one more period)
      batch_K_blocks                   a batch member's blocks first reach K"""
    t = plan_table(plan, hi) if table is None else table
    n = np.arange(hi + 1)
    col = {f: t[:, k] for k, f in enumerate(FIELDS)}
    out = {}

    def held_before(ch, i):  # how long the value before change i lasted
        return ch[i] - (ch[i - 1] if i > 0 else 1)

    ch = _changes(col["ppb"])
    if ch:
        out["ppb_leaves_min"] = ch[0]
        if len(ch) > 1 and hi - ch[-1] >= held_before(ch, len(ch) - 1):
            out["ppb_saturates"] = ch[-1]
    for form, f in (("fused", "fused_blocks"), ("launch", "launch_blocks"), ("server", "server_blocks")):
        ch = _changes(col[f])
        if not ch:
            continue
        out[form + "_two_blocks"] = _first(col[f] == 2)
        out[form + "_max"] = _first(col[f] == col[f][1:].max())
        if hi - ch[-1] > held_before(ch, len(ch) - 1):
            out[form + "_cap"] = ch[-1]
            if form == "launch" and len(ch) > 1:
                out["launch_strided"] = ch[-1] + held_before(ch, len(ch) - 1)
    out["fused_strided"] = _first(col["fused_blocks"] * col["ppb"] < n)
    out["server_walk"] = _first(col["server_blocks"] * col["ppb"] < n)
    for k in (2, 3, 9):
        out["batch_%d_blocks" % k] = _first(col["batch_blocks"] == k)
    return {k: int(b) for k, b in out.items() if b is not None and 2 <= b <= hi - 1}


def sizes_around(bounds, names=None):
    """Sorted, de-duplicated b - 1, b, b + 1 of the named boundaries (all of them by default)."""
    s = set()
    for k, b in bounds.items():
        if names is None or k in names:
            s.update((b - 1, b, b + 1))
    return sorted(x for x in s if x >= 1)


def eval_sizes(bounds):
    """Every size the evaluation sweep runs: the fixed small ones and each evaluation boundary +- 1."""
    return sorted(set(SMALL_SIZES) | set(sizes_around(bounds, EVAL_BOUNDARIES)))


def batch_member_sizes(bounds, above=None):
    """Member sizes of the ragged batch / the pairs: 0, 1, each batch boundary +- 1, and (if given) one larger member."""
    s = {0, 1} | set(sizes_around(bounds, BATCH_BOUNDARIES))
    if above:
        s.add(above)
    return sorted(s)
