"""CPU: the tile plan of hvi_cidnet_amd.image_io (pure host code) -- its geometry, its weights against the formula restated
here in fp64, every rejection, the exports, the header's two tile entry points and the errors raised before a device is touched."""
import inspect
import itertools

import numpy as np
import pytest
import torch

SIZES = [(16, 16), (37, 53), (100, 150), (24, 200), (1000, 1504)]
TILES = [16, 64, (32, 64)]


def _cases():
    for (h, w), tile in itertools.product(SIZES, TILES):
        Th, Tw = (tile, tile) if isinstance(tile, int) else tile
        for overlap in (0, 8, "half"):
            yield h, w, tile, overlap, (Th, Tw)


def _plan(h, w, tile, overlap, T):
    """the plan, with overlap 'half' = half of the smaller side of the tile the plan will use"""
    from hvi_cidnet_amd import image_io as IO
    Hp, Wp = IO.padded_size(h, w)
    t = min(min(T[0], Hp), min(T[1], Wp))
    return IO.tile_plan(h, w, tile, t // 2 if overlap == "half" else overlap), (t // 2 if overlap == "half" else overlap)


def _weights(o, t):
    """the issue's formula, fp64, rounded once"""
    out = np.empty((len(o), t), dtype=np.float64)
    for k in range(len(o)):
        l = max(0, o[k - 1] + t - o[k]) if k > 0 else 0
        r = max(0, o[k] + t - o[k + 1]) if k + 1 < len(o) else 0
        for i in range(t):
            out[k, i] = min(1.0, (i + 1) / (l + 1), (t - i) / (r + 1))
    return out.astype(np.float32)


@pytest.mark.parametrize("h,w,tile,overlap,T", list(_cases()))
def test_plan_properties(h, w, tile, overlap, T):
    from hvi_cidnet_amd import image_io as IO
    plan, ov = _plan(h, w, tile, overlap, T)
    Hp, Wp = IO.padded_size(h, w)
    th, tw = min(T[0], Hp), min(T[1], Wp)
    assert plan.size == (h, w) and plan.padded == (Hp, Wp) and plan.tile == (th, tw)
    assert plan.origins.dtype == np.int32 and plan.origins.shape == (len(plan.ys) * len(plan.xs), 2) and len(plan) == len(plan.origins)
    assert plan.origins.tolist() == [[y, x] for y in plan.ys for x in plan.xs]                   # row-major over ys x xs
    for o, t, P, a in ((plan.ys, th, Hp, plan.wy), (plan.xs, tw, Wp, plan.wx)):
        assert o[0] == 0 and o[-1] == P - t and all(b > a_ for a_, b in zip(o, o[1:]))            # inside, flush, ascending
        if t == P:
            assert o == (0,)                                                                      # the image fits: one tile
        else:
            S = t - ov
            regular = o[:-1] if (P - t) % S else o
            assert list(regular) == list(range(0, S * len(regular), S))                           # 0, S, 2S, ... while a tile fits
            assert regular[-1] + S + t > P or o[-1] == regular[-1]
        cover = np.zeros(P, dtype=np.int64)
        for y in o:
            cover[y:y + t] += 1
        assert cover.min() >= 1 and cover.max() <= 3                                              # full coverage, at most 3
        assert a.dtype == np.float32 and a.shape == (len(o), t) and (a > 0).all()
        assert np.array_equal(a, _weights(o, t))
        if [P - t - y for y in reversed(o)] == list(o):                                           # a symmetric plan
            assert np.array_equal(a, a[::-1, ::-1])
    if Hp <= T[0] and Wp <= T[1]:
        assert len(plan) == 1 and plan.tile == (Hp, Wp) and (plan.wy == 1).all() and (plan.wx == 1).all()


def test_a_symmetric_and_a_triple_cover_plan_exist_in_the_grid():
    """the properties above are conditional on what the plans are: here is what they are for two of them"""
    from hvi_cidnet_amd import image_io as IO
    p = IO.tile_plan(100, 150, 64, 32)                            # padded (104, 152)
    assert p.ys == (0, 32, 40) and p.xs == (0, 32, 64, 88)        # rows 40..63 are covered by three tiles
    assert p.wy[1, 0] == np.float32(1 / 33) and p.wy[1, 63] == np.float32(1 / 57) and p.wy[2, 0] == np.float32(1 / 57)
    s = IO.tile_plan(16, 120, 64, 8)                              # 120 = 64 + 56: two tiles, mirror images of each other
    assert s.xs == (0, 56) and np.array_equal(s.wx, s.wx[::-1, ::-1]) and s.wx[0, -1] == np.float32(1 / 9)
    assert IO.tile_plan(100, 150, 256).tile == (104, 152) and len(IO.tile_plan(100, 150, 256)) == 1
    assert IO.tile_plan(100, 150, 64, 32) is p                    # cached: the device copies are made once per plan


@pytest.mark.parametrize("args", [
    (100, 150, 60), (100, 150, (64, 20)),                         # no multiple of 8
    (100, 150, 0), (100, 150, -64), (100, 150, (64, 0)),          # non-positive tile
    (0, 150, 64), (100, -1, 64),                                  # non-positive image
    (100, 150, 64, -1),                                           # negative overlap
    (100, 150, 64, 33), (100, 150, (32, 64), 17),                 # more than half of the tile
    (2, 150, 64), (100, 3, 64), (2, 8, 64),                       # _check_reflect: pad >= side (even where one tile would do)
    (100, 150, 64, 32, 0), (100, 150, 64, 32, -8),                # multiple
    (100, 150, 64.5), (100.5, 150, 64),                           # not integers
    (100, 150, float("inf")), (float("inf"), 150, 64), (100, 150, 64, float("nan")), (100, 150, "64"), (100, 150, (64, 64, 64)),
])
def test_plan_rejections(args):
    from hvi_cidnet_amd import image_io as IO
    with pytest.raises(ValueError):
        IO.tile_plan(*args)


def test_overlap_is_only_bounded_where_something_overlaps():
    from hvi_cidnet_amd import image_io as IO
    assert len(IO.tile_plan(100, 150, 256, overlap=200)) == 1     # one tile: the overlap has nothing to bound
    assert IO.tile_plan(100, 150, 64, 32).ys == (0, 32, 40)       # exactly half is allowed
    assert IO.tile_plan(100, 150, (104, 64), 32).ys == (0,)       # one axis single, the other tiled


def test_exports_and_signatures():
    import hvi_cidnet_amd as P
    for name in ("tile_plan", "TilePlan", "ingest_tiles", "egress_tiles"):
        assert name in P.__all__ and getattr(P, name) is getattr(P.image_io, name), name
    for fn in (P.enhance_u8, P.enhance_folder):
        sig = inspect.signature(fn).parameters
        assert sig["tile"].default is None and sig["overlap"].default == 32 and sig["tile_batch"].default == 8
    assert P.EnhanceReport().tiles == []
    sig = inspect.signature(P.tile_plan).parameters
    assert sig["overlap"].default == 32 and sig["multiple"].default == 8


def test_header_declares_the_tile_entry_points():
    from hvi_cidnet_amd import _lib
    protos = _lib.parse_header()
    assert [a for _, a in protos["cidnet_image_ingest_tiles"][1]] == ["src", "h", "w", "table", "origins", "x", "n", "th", "tw", "stream"]
    assert [a for _, a in protos["cidnet_image_egress_tiles"][1]] == ["tiles", "origins_y", "ny", "origins_x", "nx", "wy", "wx", "dst",
                                                                       "h", "w", "th", "tw", "stream"]
    assert _lib.lib().raw("cidnet_abi_version")() >= 14


def test_cpu_tensors_raise_before_the_library_is_loaded(monkeypatch):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import image_io as IO

    def no_lib():
        raise AssertionError("the library was loaded for a CPU tensor")
    monkeypatch.setattr(IO, "lib", no_lib)
    plan = P.tile_plan(16, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.ingest_tiles(torch.zeros((16, 16, 3), dtype=torch.uint8), plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.egress_tiles(torch.zeros((1, 3, 16, 16)), plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.enhance_u8(torch.nn.Identity(), torch.zeros((16, 16, 3), dtype=torch.uint8), tile=16)


def test_the_image_independent_checks_stand_alone():
    """enhance_folder runs them before it starts a worker (tests/test_tiles_gpu.py): tile, overlap and multiple without an image"""
    from hvi_cidnet_amd import image_io as IO
    assert IO._check_tile(64, 32) == (64, 64, 32, 8) and IO._check_tile((32, 64.0), 0, 4) == (32, 64, 0, 4)
    for bad in ((20, 32), (64, -1), ((64, 0), 32), (float("inf"), 32), (64, float("nan")), ((64,), 32), (64, 32, 0), (True, 32)):
        with pytest.raises(ValueError):
            IO._check_tile(*bad)
