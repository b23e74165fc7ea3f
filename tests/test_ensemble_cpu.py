"""CPU: the argument checks of the self-ensemble mode -- they run before anything touches a device -- and the two exports of
csrc/ensemble.hip in the header and the library."""
import ctypes
import inspect
import os

import pytest
import torch


@pytest.mark.parametrize("ensemble", [0, 3, 16, "8"])
def test_other_ensemble_values_are_value_errors(ensemble, tmp_path):
    import hvi_cidnet_amd as P
    imgs = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        P.enhance_u8(None, imgs, ensemble=ensemble)
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        P.enhance_folder(None, str(tmp_path), str(tmp_path / "out"), ensemble=ensemble)
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        P.enhance(None, torch.zeros(3, 16, 16), ensemble=ensemble)
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        P.evaluate(None, [(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))], ensemble=ensemble)
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        P.evaluate_unpaired(None, [torch.zeros(3, 96, 96)], P.metrics.NiqeParams(None, None, None), ensemble=ensemble)
    assert not (tmp_path / "out").exists()                       # raised before the output directory was made


def test_ensemble_with_tiles_is_a_value_error(tmp_path):
    import hvi_cidnet_amd as P
    imgs = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="tile"):
        P.enhance_u8(None, imgs, ensemble=4, tile=16)
    with pytest.raises(ValueError, match="tile"):
        P.enhance_folder(None, str(tmp_path), str(tmp_path / "out"), ensemble=4, tile=16)
    assert P.image_io._check_ensemble(1, tile=16) == (1, 0)      # the tiled mode itself is untouched
    assert [P.image_io._check_ensemble(e) for e in (1, 2, 4, 8)] == [(1, 0), (2, 0), (4, 0), (4, 4)]


def test_cpu_tensors_are_refused():
    import hvi_cidnet_amd as P
    x = torch.zeros((1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.image_io.ensemble_views(x, 0, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.image_io.ensemble_merge(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.image_io.ensemble_merge(x, x, na=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.enhance_u8(None, torch.zeros((1, 16, 16, 3), dtype=torch.uint8), ensemble=8)


def test_header_declares_and_library_exports_the_two_entry_points():
    from hvi_cidnet_amd import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("cidnet_ensemble_views", 9), ("cidnet_ensemble_merge", 10)):
        assert name in protos, name
        ret, sig = protos[name]
        assert ret is ctypes.c_int and len(sig) == nargs and sig[-1] == (ctypes.c_void_p, "stream"), (name, sig)
        assert hasattr(dll, name), f"libcidnet_hip.so lacks {name}"
    assert [n for _, n in protos["cidnet_ensemble_views"][1]] == ["x", "y", "B", "C", "H", "W", "first", "count", "stream"]
    assert [n for _, n in protos["cidnet_ensemble_merge"][1]] == ["ya", "na", "yb", "nb", "out", "B", "C", "H", "W", "stream"]
    assert _lib.lib().raw("cidnet_abi_version")() >= 17


def test_the_entry_points_reject_bad_arguments_without_a_device():
    """the argument checks run on the host before any launch: the status codes of the header's block"""
    from hvi_cidnet_amd import _lib
    views, merge = _lib.lib().raw("cidnet_ensemble_views"), _lib.lib().raw("cidnet_ensemble_merge")
    p = ctypes.c_void_p(4096)                                    # never dereferenced: every call below is rejected
    assert views(None, p, 1, 3, 8, 8, 0, 4, None) == -1 and views(p, None, 1, 3, 8, 8, 0, 4, None) == -1
    for args in ((1, 3, 8, 8, 0, 0), (1, 3, 8, 8, 2, 3), (1, 3, 8, 8, 6, 3), (1, 3, 8, 8, -1, 1), (16384, 3, 8, 8, 0, 4),
                 (0, 3, 8, 8, 0, 4), (1, 0, 8, 8, 0, 4), (1, 3, 0, 8, 0, 4), (1, 3, 8, 0, 0, 4)):
        assert views(p, p, *args, None) == -2, args
    assert merge(None, 4, p, 4, p, 1, 3, 8, 8, None) == -1 and merge(p, 4, p, 4, None, 1, 3, 8, 8, None) == -1
    for na, yb, nb, dims in ((0, p, 4, (1, 3, 8, 8)), (5, p, 4, (1, 3, 8, 8)), (4, p, 5, (1, 3, 8, 8)), (4, p, -1, (1, 3, 8, 8)),
                             (4, None, 1, (1, 3, 8, 8)), (4, p, 0, (1, 3, 8, 8)), (1, None, 0, (65536, 3, 8, 8)),
                             (4, p, 4, (0, 3, 8, 8)), (4, p, 4, (1, 3, 8, -1))):
        assert merge(p, na, yb, nb, p, *dims, None) == -2, (na, nb, dims)


def test_every_image_producing_entry_point_takes_ensemble_and_defaults_to_one():
    import hvi_cidnet_amd as P
    for fn in (P.enhance_u8, P.enhance_folder, P.enhance, P.evaluate, P.evaluate_unpaired):
        assert inspect.signature(fn).parameters["ensemble"].default == 1, fn.__name__
    for cls in (P.EnhanceReport, P.metrics.EvalResult, P.metrics.UnpairedResult):
        assert cls.__dataclass_fields__["ensemble"].default == 1, cls.__name__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "tools", "enhance.py")).read()
    assert "--ensemble" in src and "ensemble=a.ensemble" in src
