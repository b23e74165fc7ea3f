"""CPU: the host side of hvi_cidnet_amd.image_io -- the batching / rank-sharding plan of enhance_folder as a pure function, the
padded size, the exports, the header's two new entry points, and the errors raised before anything reaches a device."""
import re

import pytest
import torch


def test_plan_keeps_the_order_and_batches_runs_of_equal_size():
    from hvi_cidnet_amd import image_io as IO
    a, b, c = (400, 600), (384, 384), (600, 400)
    sizes = [a, a, a, b, a, a, c, c, c, c, c]
    assert list(IO.plan_batches(sizes, batch_size=1)) == [[i] for i in range(len(sizes))]
    assert list(IO.plan_batches(sizes, batch_size=4)) == [[0, 1, 2], [3], [4, 5], [6, 7, 8, 9], [10]]
    assert list(IO.plan_batches(sizes, batch_size=2)) == [[0, 1], [2], [3], [4, 5], [6, 7], [8, 9], [10]]
    assert list(IO.plan_batches([], batch_size=4)) == []
    # equal padded sizes are not enough: one launch ingests one image size
    assert list(IO.plan_batches([(36, 52), (33, 50), (40, 56)], batch_size=4)) == [[0], [1], [2]]


def test_plan_is_lazy_one_image_ahead():
    from hvi_cidnet_amd import image_io as IO
    seen = []

    def sizes():
        for i, s in enumerate([(8, 8)] * 3 + [(9, 9)] * 2):
            seen.append(i)
            yield s
    it = IO.plan_batches(sizes(), batch_size=2)
    assert next(it) == [0, 1] and seen == [0, 1, 2]                         # yielded once the image after it has been seen
    assert next(it) == [2] and seen == [0, 1, 2, 3]
    assert list(it) == [[3, 4]]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_ranks_take_every_world_th_image(world):
    from hvi_cidnet_amd import image_io as IO
    names = [f"{i:03d}.png" for i in range(11)]
    sizes = [(8, 8 + 8 * (i // 4)) for i in range(11)]
    seen = []
    for rank in range(world):
        mine = list(IO.shard(len(names), rank, world))
        assert mine == [i for i in range(len(names)) if i % world == rank]
        batches = list(IO.plan_batches([sizes[i] for i in mine], rank, world, batch_size=3))
        assert [i for b in batches for i in b] == mine                       # the order of the names
        for b in batches:
            assert len(b) <= 3 and len({sizes[i] for i in b}) == 1
        seen += mine
    assert sorted(seen) == list(range(len(names)))
    with pytest.raises(ValueError):
        IO.shard(4, 2, 2)


def test_padded_size_is_pad_to_multiples_arithmetic():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import image_io as IO
    for h, w in [(8, 8), (9, 13), (10, 23), (33, 50), (16, 24), (5, 9), (400, 600), (1, 1)]:
        H, W = ((h + 8) // 8) * 8, ((w + 8) // 8) * 8
        assert IO.padded_size(h, w) == (H if h % 8 else h, W if w % 8 else w)
    assert tuple(P.pad_to_multiple(torch.zeros(1, 3, 9, 16))[0].shape[-2:]) == IO.padded_size(9, 16) == (16, 16)
    with pytest.raises(ValueError):
        IO.padded_size(8, 8, 0)


def test_exports():
    import hvi_cidnet_amd as P
    for name in ("image_io", "ingest", "egress", "enhance_u8", "enhance_folder"):
        assert name in P.__all__ and hasattr(P, name), name
    assert P.ingest is P.image_io.ingest and P.enhance_folder is P.image_io.enhance_folder
    assert callable(P.enhance)                                               # the function of that name is still the function
    rep = P.image_io.EnhanceReport()
    assert rep.names == [] and rep.sizes == [] and rep.batches == [] and rep.seconds == {}


def test_header_declares_the_image_entry_points():
    from hvi_cidnet_amd import _lib
    protos = _lib.parse_header()
    for name, n_args in (("cidnet_image_ingest", 10), ("cidnet_image_egress", 9)):
        assert name in protos and len(protos[name][1]) == n_args, name
    assert [a for _, a in protos["cidnet_image_ingest"][1]] == ["src", "src_bs", "table", "x", "B", "h", "w", "Hp", "Wp", "stream"]
    assert [a for _, a in protos["cidnet_image_egress"][1]] == ["x", "dst", "dst_bs", "B", "Hp", "Wp", "h", "w", "stream"]
    hv = int(re.search(r"#define\s+CIDNET_ABI_VERSION\s+(\d+)", open(_lib.HEADER).read()).group(1))
    assert hv >= 11 and _lib.lib().raw("cidnet_abi_version")() == hv


def test_cpu_tensors_raise_before_the_library_is_loaded(monkeypatch):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import image_io as IO

    def no_lib():
        raise AssertionError("the library was loaded for a CPU tensor")
    monkeypatch.setattr(IO, "lib", no_lib)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.ingest(torch.zeros((8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.ingest(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), gamma=1.4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.egress(torch.zeros((1, 3, 8, 8)), (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.enhance_u8(torch.nn.Identity(), torch.zeros((8, 8, 3), dtype=torch.uint8))


def test_evaluate_functions_take_save_dir():
    import inspect
    import hvi_cidnet_amd as P
    for fn in (P.evaluate, P.evaluate_unpaired):
        assert inspect.signature(fn).parameters["save_dir"].default is None
