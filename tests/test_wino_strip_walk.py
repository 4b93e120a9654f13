"""CPU: the strip walk of the Winograd tile kernels (tests/wino_strip_walk.py restates conv_wino.hip's scheduler) covers every tile of a
launch exactly once -- whole, or as its four quadrant units -- at every CU count, with and without units, for whole frames and for a
row band that starts at tile 378; and the checker that says so fails for three one-term slips of the walk (negative controls).
tests/test_gpu_wino_strips.py ties the restatement to the kernels themselves."""
import pytest

import wino_strip_walk as sw

# every count up to 1100 (one round up to four rounds on 256 CUs, every remainder mod 8 and every `left`), then 480x854, 720p, 1080p, 2160p
TCOUNTS = list(range(1, 1101)) + [1620, 3600, 8160, 32400]


@pytest.mark.parametrize('units', [True, False], ids=['units', 'no units (MS)'])
@pytest.mark.parametrize('cus', [256, 304, 64])
@pytest.mark.parametrize('tile0', [0, 378])
def test_every_tile_is_walked_exactly_once(tile0, cus, units):
    for tcount in TCOUNTS:
        wk = sw.walk(tcount, tile0, cus, units)
        assert wk.grid == sw.grid_of(tcount, cus) == len(wk.tiles) == len(wk.units)
        errs = sw.coverage_errors(wk, tcount, tile0)
        assert not errs, (tcount, tile0, cus, units, errs)
        if not units:
            assert not any(wk.units) and not wk.classes & {'B', 'B-idle'}


def test_the_classes_of_the_frames_the_suite_names():
    """256 CUs: the sizes DESIGN.md's test list and tests/test_gpu_wino_strips.py speak of"""
    c = lambda n, **kw: (sw.walk(n, **kw).classes, sw.walk(n, **kw).max_rounds)      # noqa: E731
    assert c(3) == ({'flat'}, 1)
    assert c(63) == ({'A', 'B', 'B-idle'}, 1)                   # 100x132
    assert c(324) == ({'B', 'C'}, 1)                            # 277x283: left = 8 fills all 32 slots; left = 9 is a partial round
    assert c(506) == ({'A', 'C'}, 2)                            # 340x361
    assert c(513) == ({'A', 'B', 'B-idle'}, 2)                  # 297x421
    assert c(1620) == ({'C'}, 6)                                # 480x854
    assert c(510) == ({'A', 'C'}, 2)                            # 270x480
    assert c(3600) == ({'B', 'B-idle'}, 14)                     # 720p
    assert c(8160) == ({'C'}, 31)                               # 1080p
    assert c(3600, units=False) == ({'C'}, 14)
    wk = sw.walk(324)
    # bands 0-3 hold 41 tiles, band x = 4..7 the 40 tiles from 164 + 40 (x - 4): its last 8 are unit tiles
    assert sorted(q for q in wk.units if q) == [(164 + 40 * x + 32 + i, q) for x in range(4) for i in range(8) for q in range(4)]
    # 100x132: the last tile column is 4 pixels wide, the last tile row 4 pixels high
    assert sw.unit_inside((62, 0), 100, 132) and not sw.unit_inside((62, 1), 100, 132) and not sw.unit_inside((62, 2), 100, 132)
    assert sw.unit_inside((8, 2), 100, 132) and not sw.unit_inside((8, 3), 100, 132) and sw.unit_inside((61, 1), 100, 132)


@pytest.mark.parametrize('variant,tcount', list(zip(sw.VARIANTS, (63, 324, 513))))
def test_the_checker_bites_on_a_slipped_walk(variant, tcount):
    """negative controls: `xcd <= br` for `xcd < br` gives a band one tile too many (63 tiles: tile 63 does not exist); `4 * left <=
    tstep + 4` takes 36 units for 32 blocks (324 tiles); `qtile = tend + (slot & 3)` puts a band's units on four tiles (513 tiles)"""
    assert not sw.coverage_errors(sw.walk(tcount), tcount)
    assert sw.coverage_errors(sw.walk(tcount, variant=variant), tcount)
    assert sw.coverage_errors(sw.walk(tcount, 378, variant=variant), tcount, 378)
    # common frame sizes: 480x854 and 720p see the first slip, 720p the third
    assert sw.coverage_errors(sw.walk(1620, variant='xcd<=br'), 1620) and sw.coverage_errors(sw.walk(3600, variant='xcd<=br'), 3600)
    assert sw.coverage_errors(sw.walk(3600, variant='qtile=tend+(slot&3)'), 3600)
