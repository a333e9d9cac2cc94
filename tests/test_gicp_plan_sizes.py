"""CPU: the size chooser of tests/test_gicp_gpu_plans.py (tests/gicp_plan_sizes.py) against a stub plan whose break points
are known by construction -- a chooser that lost a boundary would silently shrink the GPU sweep."""
import gicp_plan_sizes as gps


def stub_plan(n):
    """A toy library: 8 queries per kNN block, at most 40 blocks; 32 per correspondence block, at most 20; 10 points per
    functor block, at most 20; 10 per server block, at most 9."""
    ceil = lambda a, b: -(-a // b)
    return dict(knn_blocks=max(1, min(40, ceil(n, 8))), correspond_blocks=max(1, min(20, ceil(n, 32))),
                functor_blocks=max(1, min(20, ceil(n, 10))), server_blocks=max(1, min(9, ceil(n, 10))))


HI = 700
# worked out by hand from the stub's description (not by running the chooser): K blocks first at (K - 1) * per_block + 1
FUNCTOR = {1: 1, 2: 11, 7: 61, 8: 71, 9: 81, 16: 151, 17: 161}
SERVER = {1: 1, 2: 11, 7: 61, 8: 71, 9: 81}          # capped at 9: 16 and 17 blocks never occur
KNN = {1: 1, 2: 9, 7: 49, 8: 57, 9: 65, 16: 121, 17: 129}
CORRESPOND = {1: 1, 2: 33, 7: 193, 8: 225, 9: 257, 16: 481, 17: 513}
CAPS = dict(knn_blocks=(313, 8),          # 39 * 8 + 1: the fortieth block; 40 * 8 + 1 = 321 = 313 + 8 is the first strided size
            correspond_blocks=(609, 32),  # 19 * 32 + 1
            functor_blocks=(191, 10),     # 19 * 10 + 1
            server_blocks=(81, 10))       # 8 * 10 + 1


def test_chooser_finds_every_break_point_of_the_stub():
    assert gps.block_boundaries(stub_plan, "functor_blocks", HI) == FUNCTOR
    assert gps.block_boundaries(stub_plan, "server_blocks", HI) == SERVER
    assert gps.block_boundaries(stub_plan, "knn_blocks", HI) == KNN
    assert gps.block_boundaries(stub_plan, "correspond_blocks", HI) == CORRESPOND
    for field in gps.FIELDS:
        assert gps.cap_boundary(stub_plan, field, HI) == CAPS[field], field
        for b in gps.block_boundaries(stub_plan, field, HI).values():
            assert gps.is_boundary(stub_plan, field, b) and (b == 1 or not gps.is_boundary(stub_plan, field, b - 1))
            assert not gps.is_boundary(stub_plan, field, b + 1)
    assert gps.first_reaching(stub_plan, "knn_blocks", 41, HI) is None
    assert gps.first_reaching(stub_plan, "knn_blocks", 40, HI) == 313 and gps.first_reaching(stub_plan, "knn_blocks", 1, HI) == 1


def test_chooser_returns_every_break_point_plus_and_minus_one():
    sizes = gps.functor_sweep_sizes(stub_plan, HI)
    for b in set(FUNCTOR.values()) | set(SERVER.values()):
        for d in (-1, 0, 1):
            assert b + d in sizes or b + d < 1, (b, d)
    # 7 distinct boundaries (the server's are among the functor's) x 3 = 21 sizes, less size 0
    assert sizes == [1, 2, 10, 11, 12, 60, 61, 62, 70, 71, 72, 80, 81, 82, 150, 151, 152, 160, 161, 162]
    assert gps.cap_sizes(stub_plan, "functor_blocks", HI) == [190, 191, 192, 201, 202]
    assert gps.cap_sizes(stub_plan, "server_blocks", HI) == [80, 81, 82, 91, 92]
    assert gps.cap_sizes(stub_plan, "knn_blocks", HI) == [312, 313, 314, 321, 322]
    assert gps.around([1, 9, 10]) == [1, 2, 8, 9, 10, 11]


def test_chooser_reports_only_what_the_plan_reaches():
    """A plan that never changes, a count the grid jumps over, a range that ends before the cap has held for long: none of
    them yields a boundary -- and the end of the range is not mistaken for a cap."""
    flat = lambda n: dict(knn_blocks=1, correspond_blocks=1, functor_blocks=1, server_blocks=1)
    for field in gps.FIELDS:
        assert gps.block_boundaries(flat, field, 300) == {1: 1}
        assert gps.cap_boundary(flat, field, 300) is None and gps.cap_sizes(flat, field, 300) == []
    jumps = lambda n: dict(flat(n), functor_blocks=1 if n < 50 else 3)
    assert gps.block_boundaries(jumps, "functor_blocks", 300) == {1: 1}
    assert gps.cap_boundary(jumps, "functor_blocks", 300) == (50, 49)
    # the correspondence grid reaches its twentieth block at 609; by 650 that value has held for 41 sizes, less than two
    # periods of 32: still growing for all the chooser can tell
    assert gps.cap_boundary(stub_plan, "correspond_blocks", 650) is None
    assert gps.cap_boundary(stub_plan, "correspond_blocks", 674) == (609, 32)
    # a boundary whose b + 1 would lie beyond the range is not reported
    assert 17 not in gps.block_boundaries(stub_plan, "functor_blocks", 161) and gps.block_boundaries(stub_plan, "functor_blocks", 162)[17] == 161
    # a capped grid (NDT_GICP_MAX_BLOCKS=3): the counts above the cap are gone, the cap is where the third block appears
    capped = lambda n: {k: min(v, 3) for k, v in stub_plan(n).items()}
    assert gps.block_boundaries(capped, "functor_blocks", HI) == {1: 1, 2: 11}
    assert gps.cap_boundary(capped, "functor_blocks", HI) == (21, 10)
