"""The strip walk of the persistent Winograd tile kernels as a pure function (no GPU, no torch): which block walks which whole tiles and
which quadrant unit, restated from the two places that decide it

  * launch_wino_rows (pnp_vcve_amd/csrc/conv_wino.hip:1786-1787): grid = min(ntiles, CUs), rounded down to a multiple of 8 once it is
    at least 8; every body is launched with w.quad = 1 (:1768), the multi-source one included -- its kernel ignores it;
  * wino_tile_body (conv_wino.hip:150-176): the strip of a block.  gridDim.x a multiple of 8: XCD x = blockIdx & 7 owns the band
    [xbeg, tend) of tcount >> 3 tiles, one more for x < (tcount & 7) (:155-157); slot = blockIdx >> 3 walks xbeg + slot, + tstep, ...
    with tstep = gridDim.x >> 3 (:158-159); the `left` tiles beyond the band's whole rounds become 4 * left quadrant units, one per
    slot, iff 0 < left and 4 * left <= tstep and the body is not the multi-source one (:163-170).  Any other gridDim.x (< 8 tiles):
    block b walks tile0 + b, + gridDim.x, ... (:171-175).  A block whose first tile is not below tend returns (:176).

tests/test_wino_strip_walk.py checks that the restatement covers every tile exactly once; tests/test_gpu_wino_strips.py ties it to
the kernels block by block through their trace words and picks its frames from the classes it reports.

Classes of a band (a launch's set is the union over its bands):
  flat    the launch has fewer than 8 blocks: no bands, one tile per block
  A       left == 0: whole rounds only
  B       1 <= left <= tstep / 4: the leftover tiles run as quadrant units
  B-idle  a B band with 4 * left < tstep: some of its blocks get no unit (named next to B, not instead of it)
  C       left > 0 otherwise: the leftover tiles run as one more, partial, round of whole tiles"""
import collections

Walk = collections.namedtuple('Walk', 'grid tiles units classes max_rounds')
Walk.__doc__ = """grid: blocks launched.  tiles[b]: the whole tiles block b walks, in order (a range).  units[b]: its quadrant unit
(tile, quad) or None.  classes: the set of band classes present.  max_rounds: the most whole rounds (band tiles // tstep) of any band
(flat: 1)."""

# the three slips the CPU test must catch (negative controls): one per term of the walk a handful of tiles hangs on
VARIANTS = ('xcd<=br', '4*left<=tstep+4', 'qtile=tend+(slot&3)')


def grid_of(tcount, cus=256):
    """launch_wino_rows, conv_wino.hip:1786-1787"""
    grid = min(tcount, cus)
    if grid >= 8:
        grid -= grid % 8
    return grid


def walk(tcount, tile0=0, cus=256, units=True, variant=None):
    """The launch over tiles [tile0, tile0 + tcount) on a device of `cus` CUs; units=False: the multi-source body (never takes units).
    variant: None = the kernel's walk; one of VARIANTS = that walk with one term slipped."""
    assert tcount >= 1 and (variant is None or variant in VARIANTS)
    grid = grid_of(tcount, cus)
    tiles, unit, classes, max_rounds = [], [], set(), 1
    if grid & 7:                                                        # :171-175
        classes.add('flat')
        for b in range(grid):
            tiles.append(range(tile0 + b, tile0 + tcount, grid))
            unit.append(None)
        return Walk(grid, tiles, unit, classes, max_rounds)
    tstep = grid >> 3                                                   # :159
    bq, br = tcount >> 3, tcount & 7                                    # :155
    for b in range(grid):
        xcd, slot = b & 7, b >> 3                                       # :154
        more = xcd <= br if variant == 'xcd<=br' else xcd < br
        xbeg = tile0 + (xcd * (bq + 1) if more else br * (bq + 1) + (xcd - br) * bq)      # :156
        tend = xbeg + bq + (1 if more else 0)                           # :157
        nband = tend - xbeg                                             # :163
        rounds, left = nband // tstep, nband % tstep
        q = None
        fits = 4 * left <= tstep + (4 if variant == '4*left<=tstep+4' else 0)
        if units and rounds >= 1 and left > 0 and fits:                 # :164
            tend = xbeg + rounds * tstep                                # :165
            if slot < 4 * left:                                         # :166
                q = (tend + ((slot & 3) if variant == 'qtile=tend+(slot&3)' else (slot >> 2)), slot & 3)      # :167-168
            cls = ('B', 'B-idle') if 4 * left < tstep else ('B',)
        else:
            cls = ('A',) if left == 0 else ('C',)
        if slot == 0:
            classes.update(cls)
            max_rounds = max(max_rounds, rounds)
        tiles.append(range(xbeg + slot, tend, tstep))                   # :158, :176, the tile loop's `tile + tstep < tend`
        unit.append(q)
    return Walk(grid, tiles, unit, classes, max_rounds)


def unit_inside(unit, h, w):
    """whether the kernel works on the unit at all: its 8x8 quadrant's origin lies inside the h x w frame (conv_wino.hip:970-971)"""
    tile, quad = unit
    tiles_x = (w + 15) >> 4
    return (tile // tiles_x) * 16 + 8 * (quad >> 1) < h and (tile % tiles_x) * 16 + 8 * (quad & 1) < w


def coverage_errors(wk, tcount, tile0=0, limit=5):
    """The property a walk must have, as a list of what breaks it (empty = holds): every tile of [tile0, tile0 + tcount) is walked whole
    exactly once or appears as exactly its four units, each once; nothing outside the range appears; a block with a unit walked at least
    one whole tile (the unit's halo arrives through that tile's K loop)."""
    # the common case first, without a Python-level loop over tiles: the whole tiles and the tiles that appear as exactly units 0..3,
    # each unit once, are together exactly the range -- and no block has a unit without a whole tile
    seen, qs = [], collections.defaultdict(list)
    for ts, q in zip(wk.tiles, wk.units):
        seen.extend(ts)
        if q is not None:
            qs[q[0]].append(q[1] if len(ts) else -1)
    if all(sorted(v) == [0, 1, 2, 3] for v in qs.values()) and sorted(seen + list(qs)) == list(range(tile0, tile0 + tcount)):
        return []
    errs = []
    whole = [0] * tcount
    quads = {}
    for b, (ts, q) in enumerate(zip(wk.tiles, wk.units)):
        if len(ts):
            if ts[0] < tile0 or ts[-1] >= tile0 + tcount:
                errs.append('block %d walks tiles %d..%d outside [%d, %d)' % (b, ts[0], ts[-1], tile0, tile0 + tcount))
            for t in ts:
                if tile0 <= t < tile0 + tcount:
                    whole[t - tile0] += 1
        if q is not None:
            if not len(ts):
                errs.append('block %d has unit %r but no whole tile' % (b, q))
            if not (tile0 <= q[0] < tile0 + tcount and 0 <= q[1] < 4):
                errs.append('block %d has unit %r outside the range' % (b, q))
            else:
                quads.setdefault(q[0], []).append(q[1])
        if len(errs) >= limit:
            return errs
    for i, n in enumerate(whole):
        qs = sorted(quads.get(tile0 + i, ()))
        if not ((n == 1 and not qs) or (n == 0 and qs == [0, 1, 2, 3])):
            errs.append('tile %d: walked whole %d times, units %r' % (tile0 + i, n, qs))
            if len(errs) >= limit:
                break
    assert errs, 'the two statements of the property disagree'
    return errs
