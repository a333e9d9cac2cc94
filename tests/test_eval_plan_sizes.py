"""CPU: the size chooser of tests/test_gpu_eval_plans.py (tests/eval_plan_sizes.py) against a stub plan whose break points
are known by construction -- a chooser that lost a boundary would silently shrink the GPU sweep."""
import eval_plan_sizes as eps


def stub_plan(n):
    """A toy device: 4 CUs, 16..64 points per block in steps of 8, one-launch grid capped at 8 blocks, separate kernels 32
    points per block capped at 10 blocks, server one block per CU, batch runs of 50 points."""
    ceil = lambda a, b: -(-a // b)
    ppb = max(16, min(64, ceil(ceil(n, 4), 8) * 8))
    return dict(ppb=ppb, fused_blocks=max(1, min(8, ceil(n, ppb))), launch_blocks=max(1, min(10, ceil(n, 32))),
                server_blocks=max(1, min(4, ceil(n, ppb))), batch_blocks=max(1, ceil(n, 50)))


# worked out by hand from the stub's description (not by running the chooser)
EXPECTED = dict(
    ppb_leaves_min=65,        # ceil(65 / 4) = 17 -> 24 points per block
    ppb_saturates=225,        # ceil(225 / 4) = 57 -> 64
    fused_two_blocks=17, fused_max=449, fused_cap=449,   # 7 * 64 + 1: the eighth block
    fused_strided=513,        # 8 * 64 + 1
    launch_two_blocks=33, launch_max=289, launch_cap=289,  # 9 * 32 + 1: the tenth block
    launch_strided=321,       # 10 * 32 + 1
    server_two_blocks=17, server_max=49,  # 3 * 16 + 1: the fourth block
    server_cap=73,            # 65 points: 3 blocks of 24; 73: four again, and four from there on
    server_walk=257,          # 4 * 64 + 1
    batch_2_blocks=51, batch_3_blocks=101, batch_9_blocks=401)
HI = 700


def test_chooser_finds_every_break_point_of_the_stub():
    got = eps.boundaries(stub_plan, HI)
    assert got == EXPECTED
    assert set(got) == set(eps.EVAL_BOUNDARIES) | set(eps.BATCH_BOUNDARIES)


def test_chooser_returns_every_break_point_plus_and_minus_one():
    b = eps.boundaries(stub_plan, HI)
    sizes = eps.eval_sizes(b)
    for name in eps.EVAL_BOUNDARIES:
        for d in (-1, 0, 1):
            assert EXPECTED[name] + d in sizes, (name, d)
    for s in eps.SMALL_SIZES:
        assert s in sizes
    assert any(s % 8 for s in eps.SMALL_SIZES if s > 65)
    # 11 distinct boundaries x 3 = 33 sizes, plus the 7 fixed ones, of which 64 and 65 are ppb_leaves_min - 1 and itself
    distinct = {EXPECTED[k] for k in eps.EVAL_BOUNDARIES}
    assert len(distinct) == 11 and len(sizes) == 33 + 7 - 2
    members = eps.batch_member_sizes(b, above=555)
    assert members == [0, 1, 50, 51, 52, 100, 101, 102, 400, 401, 402, 555]


def test_chooser_reports_only_what_the_plan_reaches():
    """A plan that never changes (a forced ppb, a range that ends before a cap) yields no boundary of that kind -- and the
    end of the range is not mistaken for a cap."""
    flat = lambda n: dict(ppb=64, fused_blocks=1, launch_blocks=1, server_blocks=1, batch_blocks=1)
    assert eps.boundaries(flat, 300) == {"fused_strided": 65, "server_walk": 65}  # one block of 64: strided from 65 on
    short = eps.boundaries(stub_plan, 300)   # launch grid still growing at 300 (cap at 289 held for only 11 sizes)
    assert "launch_cap" not in short and "launch_strided" not in short and "fused_cap" not in short
    assert short["ppb_saturates"] == 225 and short["server_walk"] == 257 and short["server_cap"] == 73
    assert "batch_9_blocks" not in short
