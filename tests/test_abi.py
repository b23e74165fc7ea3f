"""CPU checks of the C-ABI boundary: the library builds for gfx950, loads, and exports every symbol
that include/cidnet_hip.h declares (no kernel is launched here)."""
import ctypes
import os

import pytest


def test_header_parses_and_library_exports_every_symbol():
    from hvi_cidnet_amd import _lib
    protos = _lib.parse_header()
    assert "cidnet_hvit_fwd" in protos and "cidnet_phvit_bwd" in protos
    assert os.path.exists(_lib.LIB_PATH), "run `python hvi-cidnet_amd/build.py`"
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(dll, name), f"libcidnet_hip.so lacks {name}"
    assert _lib.lib().raw("cidnet_abi_version")() >= 1


def test_shipped_library_has_no_debug_state():
    """include/cidnet_hip.h promises stateless, re-entrant entry points: the timing-study switches
    (cidnet_debug_*) exist only in -DCIDNET_DEBUG builds, never in the in-tree library"""
    from hvi_cidnet_amd import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cidnet_debug_pw_flags", "cidnet_debug_dw_rows", "cidnet_debug_c3_flags", "cidnet_debug_c3_phases", "cidnet_debug_c3xw_flags"):
        assert not hasattr(dll, name), f"{name} exported by the production library"
    assert not any(n.startswith("cidnet_debug") for n in _lib.parse_header())


def test_dw_tiling_query_contract():
    """cidnet_dw_tiling (host only, launches nothing): the strips cover H exactly once, heights stay inside 4..24 (or H
    itself below 4), strips taller than 8 rows are taken only while the launch keeps the family's lane count, and bad
    arguments are the library's argument error"""
    from hvi_cidnet_amd import _lib
    q = _lib.lib().raw("cidnet_dw_tiling")
    min_lanes = (917504, 524288, 655360, 262144)

    def tiling(family, planes, H, W):
        r, n, c = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
        assert q(family, planes, H, W, ctypes.byref(r), ctypes.byref(n), ctypes.byref(c)) == 0
        return r.value, n.value, c.value

    tall = set()
    for family in range(4):
        for planes in (1, 2, 190, 760, 1520, 4370, 13108, 45876):
            for H in (1, 2, 3, 4, 5, 7, 8, 9, 23, 24, 25, 49, 68, 100, 400):
                for W in (1, 3, 7, 8, 9, 37, 150, 600):
                    rows, nstrips, chunks = tiling(family, planes, H, W)
                    assert rows * nstrips >= H > rows * (nstrips - 1), (family, planes, H, W, rows, nstrips)
                    assert 4 <= rows <= 24 or (H < 4 and rows == H), (family, planes, H, W, rows)
                    nx4 = (W + 3) // 4
                    if planes * nstrips * nx4 < min_lanes[family]:
                        assert rows <= 8, (family, planes, H, W, rows)
                    if rows > 8:
                        tall.add(family)
                    items = nstrips * nx4
                    assert chunks == (1 if family < 2 else max(1, -(-items // 1024))), (family, planes, H, W, chunks)
    assert tall == {0, 1, 2, 3}                                   # the sweep does reach the tall strips of every family
    assert tiling(3, 8 * 95, 400, 600) == (24, 17, 3)             # the training shape: a ragged last strip of 16 rows
    r, n, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ok = (ctypes.byref(r), ctypes.byref(n), ctypes.byref(c))
    for bad in ((-1, 4, 8, 8), (4, 4, 8, 8), (0, 0, 8, 8), (0, -3, 8, 8), (1, 4, 0, 8), (2, 4, 8, 0), (3, 4, -1, 8)):
        assert q(*bad, *ok) == -1, bad
    for i in range(3):
        ptrs = list(ok)
        ptrs[i] = None
        assert q(0, 4, 8, 8, *ptrs) == -1


_C3_FIELDS = (("thin", "MT", "LEFT", "nmb", "LOGX", "tpb", "narrow", "ntiles", "xt", "gy"),
              ("path", "MT", "LEFT", "nmb", "nfull", "ngrp", "rr", "last", "chunks", "nitems"),
              ("kside", "rows", "nstrips", "last", "lds"), ("chunks", "rows", "nstrips", "last"),
              ("tiles_x", "tiles_y", "mchunks", "kchunks", "nwork", "grid", "remap", "maxitems"),
              ("pairs", "nblk", "ntiles", "nt_min", "nt_max"))


def _c3_tiling(kind, B, M, K, H, W, levels=3):
    """cidnet_conv3x3_tiling -> (status, {field: value}); the buffer is prefilled so that unwritten fields show"""
    from hvi_cidnet_amd import _lib
    out = (ctypes.c_int * 10)(*([-7] * 10))
    rc = _lib.lib().raw("cidnet_conv3x3_tiling")(kind, B, M, K, H, W, levels, out, 10)
    vals = list(out)
    assert vals[len(_C3_FIELDS[kind]):] == [-7] * (10 - len(_C3_FIELDS[kind]))          # never past its own fields
    if rc != 0:
        assert vals == [-7] * 10                                                       # nothing written on an error
    return rc, dict(zip(_C3_FIELDS[kind], vals))


_C3_M = (1, 3, 4, 5, 12, 13, 17, 21, 24, 29, 32, 33, 36, 37, 48, 49, 50, 64, 65, 72, 97, 144, 145, 256, 257)
_C3_PLANES = [(1, 1), (1, 9), (2, 7), (3, 8), (8, 16), (9, 16), (17, 16), (5, 13), (9, 63), (23, 65), (33, 40), (57, 70),
              (100, 150), (273, 300), (417, 400)]


def test_conv3x3_tiling_fp32_forward_contract():
    """kind 0: the m-blocks cover M with MT + LEFT <= 3 accumulator sets, the tiles cover the plane exactly once, a block
    walks tpb row tiles only while the weight panel stays resident (K <= 36), W < 8 is the NARROW instantiation"""
    seen = set()
    for M in _C3_M:
        for K in (1, 4, 5, 12, 36, 37, 72):
            for B in (1, 3):
                for H, W in _C3_PLANES:
                    rc, t = _c3_tiling(0, B, M, K, H, W)
                    assert rc == 0
                    what = (B, M, K, H, W, t)
                    assert t["thin"] == int((M <= 4 and K <= 256) or (K <= 4 and M <= 256)), what
                    mb = 16 * t["MT"] + 4 * t["LEFT"]
                    assert t["MT"] >= 1 and 0 <= t["LEFT"] <= 2 and t["MT"] + t["LEFT"] <= 3, what
                    assert t["nmb"] * mb >= M > (t["nmb"] - 1) * mb, what
                    assert t["LOGX"] in (2, 3, 4) and t["narrow"] == int(W < 8) and (not t["narrow"] or t["LOGX"] == 2), what
                    tw, th = 4 << t["LOGX"], 8 * (16 >> t["LOGX"])
                    assert t["xt"] * tw >= W > (t["xt"] - 1) * tw and t["ntiles"] * th >= H > (t["ntiles"] - 1) * th, what
                    assert 1 <= t["tpb"] <= (4 if K <= 36 else 1) and t["gy"] * t["tpb"] >= t["ntiles"] > (t["gy"] - 1) * t["tpb"], what
                    seen.add((t["MT"], t["LEFT"]))
                    seen.add(("tpb", t["tpb"]))
    assert {(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0), ("tpb", 1), ("tpb", 2), ("tpb", 3)} <= seen


def test_conv3x3_tiling_fp32_wgrad_contract():
    """kinds 1 and 3: the row chunks cover H exactly once, the input tiles and groups cover N, and the workspace the fields
    imply is cidnet_conv3x3_wgrad_ws_floats"""
    from hvi_cidnet_amd import _lib
    ws = _lib.lib().raw("cidnet_conv3x3_wgrad_ws_floats")
    paths = set()
    for M in _C3_M:
        for N in (1, 4, 5, 8, 12, 16, 20, 24, 28, 36, 44, 72, 256):
            for B in (1, 3):
                for H, W in _C3_PLANES:
                    rc, t = _c3_tiling(1, B, M, N, H, W)
                    assert rc == 0
                    what = (B, M, N, H, W, t)
                    thin = (M <= 4 and N <= 256) or (N <= 4 and M <= 256)
                    assert t["path"] == (2 if thin else 1 if W < 8 else 0), what
                    paths.add(t["path"])
                    assert ws(B, M, N, H, W) == B * t["chunks"] * M * N * 9, what
                    rc3, t3 = _c3_tiling(3, B, M, N, H, W)
                    assert rc3 == (0 if thin else -2), what
                    if thin:
                        nx4 = (W + 3) // 4
                        assert t3["rows"] * t3["nstrips"] >= H > t3["rows"] * (t3["nstrips"] - 1), what
                        assert t3["last"] == H - t3["rows"] * (t3["nstrips"] - 1), what
                        assert t3["chunks"] == t["chunks"] == -(-t3["nstrips"] * nx4 // 256), what
                        continue
                    mb = 16 * t["MT"] + 4 * t["LEFT"]
                    assert t["MT"] + t["LEFT"] <= 3 and t["nmb"] * mb >= M > (t["nmb"] - 1) * mb, what
                    assert 0 <= t["ngrp"] <= 2 and 16 * t["nfull"] + 4 * t["ngrp"] >= N > 16 * (t["nfull"] - 1) + 4 * t["ngrp"], what
                    nrc = -(-H // t["rr"])
                    assert 1 <= t["last"] <= t["rr"] and (nrc - 1) * t["rr"] + t["last"] == H, what
                    assert t["rr"] >= min(8, H), what
                    assert t["nitems"] == -(-W // 32) * nrc and t["chunks"] == -(-t["nitems"] // 4), what
    assert paths == {0, 1, 2}


def test_conv3x3_tiling_thin_contract():
    """kind 2: the strips cover H exactly once; the M side takes every layer with M <= 4; not a thin layer is the shape error"""
    for M in _C3_M:
        for K in (1, 2, 4, 5, 36, 85, 86, 200, 256, 257):
            for H, W in _C3_PLANES:
                rc, t = _c3_tiling(2, 2, M, K, H, W)
                what = (M, K, H, W, t)
                thin = (M <= 4 and K <= 256) or (K <= 4 and M <= 256)
                assert rc == (0 if thin else -2), what
                if not thin:
                    continue
                assert t["kside"] == int(M > 4), what
                assert t["rows"] * t["nstrips"] >= H > t["rows"] * (t["nstrips"] - 1), what
                assert t["last"] == H - t["rows"] * (t["nstrips"] - 1) and 1 <= t["last"] <= t["rows"], what
                assert t["lds"] == (M * K * 48 if M > 4 else K * M * 48 + 3 * t["rows"] * M * 1024) <= 160 * 1024, what


def test_conv3x3_tiling_bf16x3_contract():
    """kinds 4 and 5: the tiles cover the plane exactly once, the persistent grids never exceed the work, every block's tile
    count adds up to the tiles, the implied workspace is cidnet_conv3x3_wgrad_bf16x3_ws_floats, and the shape error agrees
    with the *_supported predicates"""
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    ws = L.raw("cidnet_conv3x3_wgrad_bf16x3_ws_floats")
    planes = _C3_PLANES + [(1, 4), (12, 352), (36, 480), (50, 780), (9, 5473), (400, 600)]
    many = set()
    for M in (1, 35, 36, 47, 49, 72, 100, 144, 288):
        for K in (12, 35, 36, 37, 72, 144):
            for B in (1, 2, 8):
                for H, W in planes:
                    for lv in (1, 3):
                        rc, t = _c3_tiling(4, B, M, K, H, W, lv)
                        what = (B, M, K, H, W, lv, t)
                        assert rc == (0 if L.raw("cidnet_conv3x3_bf16x3_supported")(M, K) else -2), what
                        if rc == 0:
                            assert t["tiles_x"] * 32 >= W > (t["tiles_x"] - 1) * 32 and t["tiles_y"] * 8 >= H > (t["tiles_y"] - 1) * 8, what
                            assert t["mchunks"] * 48 >= M > (t["mchunks"] - 1) * 48 and t["kchunks"] * 36 == K, what
                            assert t["nwork"] == B * t["tiles_x"] * t["tiles_y"] * t["mchunks"], what
                            assert 1 <= t["grid"] == min(t["nwork"], 1024 if lv == 1 else 512), what
                            assert t["remap"] == int(t["grid"] % 8 == 0) and t["maxitems"] == -(-t["nwork"] // t["grid"]), what
                            many.add(t["maxitems"] > 1)
                        rc, t = _c3_tiling(5, B, M, K, H, W, lv)
                        what = (B, M, K, H, W, lv, t)
                        assert rc == (0 if L.raw("cidnet_conv3x3_wgrad_bf16x3_supported")(M, K, H, W) else -2), what
                        if rc == 0:
                            assert t["pairs"] == (M // 36) * (K // 36) and 1 <= t["nblk"] <= t["ntiles"], what
                            assert t["ntiles"] == B * -(-W // 32) * -(-H // 4), what
                            nts = [(t["ntiles"] - x + t["nblk"] - 1) // t["nblk"] for x in range(t["nblk"])]      # the kernel's split
                            assert sum(nts) == t["ntiles"] and min(nts) == t["nt_min"] >= 1 and max(nts) == t["nt_max"], what
                            assert ws(B, M, K, H, W) == t["pairs"] * t["nblk"] * 108 * 108, what
    assert many == {False, True}


def test_conv3x3_tiling_bad_arguments():
    from hvi_cidnet_amd import _lib
    q = _lib.lib().raw("cidnet_conv3x3_tiling")
    out = (ctypes.c_int * 10)()
    assert q(0, 1, 12, 12, 8, 8, 3, out, 10) == 0
    for bad in ((-1, 1, 12, 12, 8, 8, 3), (6, 1, 12, 12, 8, 8, 3), (0, 0, 12, 12, 8, 8, 3), (0, 1, 0, 12, 8, 8, 3), (1, 1, 12, -1, 8, 8, 3),
                (0, 1, 12, 12, 0, 8, 3), (0, 1, 12, 12, 8, 0, 3), (4, 1, 36, 36, 8, 8, 2), (5, 1, 36, 36, 8, 8, 0)):
        assert q(*bad, out, 10) == -1, bad
    assert q(0, 1, 12, 12, 8, 8, 3, None, 10) == -1
    for kind, n in enumerate((10, 10, 5, 4, 8, 5)):
        shape = (1, 3, 36, 8, 8) if kind in (2, 3) else (1, 36, 36, 8, 8)
        assert q(kind, *shape, 3, out, n) == 0 and q(kind, *shape, 3, out, n - 1) == -1, kind


_PW_FIELDS = (("path", "launches", "MT", "LEFT", "KS", "KS2", "kc", "nkc", "tpb", "gx", "gy", "tail", "target", "lds"),
              ("MT", "NT", "nmb", "nnb", "pch", "chunks", "last", "n_red", "n_red_ps"),
              ("cpg", "KB", "MT", "WM", "chunks", "MTW", "tiles"), ("MT", "NT", "chunks", "blocks", "most"))


def _pw_plan(kind, B, M, K, HW, W=0, zw=0, xdt=0, ydt=0, epi=0):
    """cidnet_pw_plan -> (status, {field: value}); the buffer is prefilled so that unwritten fields show"""
    from hvi_cidnet_amd import _lib
    out = (ctypes.c_int * 14)(*([-7] * 14))
    rc = _lib.lib().raw("cidnet_pw_plan")(kind, B, M, K, HW, W, zw, xdt, ydt, epi, out, 14)
    vals = list(out)
    assert vals[len(_PW_FIELDS[kind]):] == [-7] * (14 - len(_PW_FIELDS[kind]))          # never past its own fields
    if rc != 0:
        assert vals == [-7] * 14                                                       # nothing written on an error
    return rc, dict(zip(_PW_FIELDS[kind], vals))


_PW_M = (1, 4, 5, 16, 17, 20, 32, 33, 36, 37, 48, 52, 64, 72, 80, 81, 95, 96, 100, 128, 144, 190, 382, 766)
_PW_K = (1, 3, 4, 36, 37, 60, 63, 64, 72, 73, 96, 97, 100, 144, 190, 320, 321, 383, 384, 385, 400, 766, 768, 769, 772, 1000)
_PW_HW = (1, 2, 3, 4, 5, 16, 61, 64, 255, 256, 257, 260, 1028, 3750, 8192, 8193, 8196, 15000, 16384, 16388, 60000, 240000, 921856)
# (MT, LEFT) instantiated per register depth (pw.hip, launch_pw_rega_of)
_PW_REGA = {9: {(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (1, 1), (2, 1), (3, 1)}, 18: {(1, 0), (2, 0), (3, 0), (5, 0), (1, 1), (2, 1)},
            24: {(1, 0), (2, 0), (3, 0), (1, 1), (2, 1)}}


def test_pw_plan_forward_contract():
    """kind 0: the grid covers the pixel tiles (groups) and the output channels exactly once, the register kernel's (MT, LEFT,
    KS) is an instantiated triple that holds all of K, a staged chunk fits 60 KB of LDS, the tail launch follows exactly for
    ragged planes (the split-K kernel checks its own lanes), a ragged plane below one tile runs the tail kernel alone, split-K
    takes two launches exactly for 384 < K <= 768 and never with a bf16 output, and the x2 epilogue never reaches split-K"""
    seen, tpbs, targets = set(), set(), set()
    for M in _PW_M:
        for K in _PW_K:
            for HW in _PW_HW:
                for B in (1, 3, 8):
                    for epi, xdt, ydt in ((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 1, 0), (2, 0, 0)):
                        W, zw = 0, 0
                        if epi == 2:
                            if HW % 16 or HW > 240000:
                                continue
                            zw = 4 if HW % 80 else 5                 # both routes: W % 4 == 0 with zw >= 4, and W = 10
                            W = 2 * zw
                            if HW % (2 * W):
                                continue
                        rc, t = _pw_plan(0, B, M, K, HW, W, zw, xdt, ydt, epi)
                        what = (B, M, K, HW, epi, xdt, ydt, t)
                        assert rc == 0, what
                        ragged = HW % 4 != 0 or HW < 4
                        ntiles = -(-HW // 256)
                        sk = t["path"] == 0
                        assert sk == (epi != 2 and 64 <= K <= 768 and (HW <= 8192 or (HW <= 16384 and K > 320))
                                      and not (K > 384 and ydt)), what
                        units = -(-HW // 64) if sk else ntiles - ragged
                        rows = 16 * t["MT"] + 4 * t["LEFT"]
                        assert 1 <= t["tpb"] <= 8, what
                        if t["path"] != 3:
                            assert t["gx"] * t["tpb"] >= units > (t["gx"] - 1) * t["tpb"], what
                            assert t["gy"] * rows >= M > (t["gy"] - 1) * rows, what
                        assert t["tail"] == int(ragged and not sk), what
                        assert (t["path"] == 3) == (ragged and HW < 256 and not sk), what
                        assert t["target"] in (512, 1024), what
                        if sk:
                            assert t["launches"] == (2 if K > 384 else 1) and not (t["launches"] == 2 and ydt), what
                            assert 1 <= t["MT"] <= 3 and t["LEFT"] == 0 and t["kc"] == 0 and t["nkc"] == 0, what
                            k1 = min(K, 384)
                            assert t["KS"] in (9, 18, 24) and 16 * t["KS"] >= k1 and (t["KS"] == 9 or 16 * (9 if t["KS"] == 18 else 18) < k1), what
                            assert (t["KS2"] == 0) == (K <= 384) and (K <= 384 or (t["KS2"] in (9, 18, 24) and 16 * t["KS2"] >= K - 384)), what
                            assert t["lds"] == 4 * t["MT"] * 16 * 64 * 4 <= 64 * 1024, what
                            seen.add((0, t["MT"], t["KS"]))
                            tpbs.add((0, t["tpb"]))
                            continue
                        assert t["launches"] == (0 if t["path"] == 3 else 1) and t["KS2"] == 0, what
                        mt = t["MT"] + t["LEFT"]                     # tiles of the LDS / tail kernel
                        lda = 16 * mt + (16 if mt % 2 == 0 else 0)
                        assert 1 <= mt <= 6 and t["kc"] % 4 == 0 and t["kc"] * lda * 4 == t["lds"] <= 60 * 1024, what
                        assert t["nkc"] == -(-K // t["kc"]) and (t["nkc"] == 1 or (t["kc"] + 4) * lda * 4 > 60 * 1024), what
                        if t["path"] == 1:
                            assert (t["MT"], t["LEFT"]) in _PW_REGA[t["KS"]] and 4 * t["KS"] >= K, what
                            assert t["gy"] == 1 or t["LEFT"] == 0, what        # the 4-row group closes a single block
                            assert epi != 2 or (W % 4 == 0 and zw >= 4), what
                            assert t["target"] == (1024 if M >= 2 * K and M * K < 50 * (M + K) else 512), what
                            targets.add(t["target"])
                        else:
                            assert t["LEFT"] == 0 and t["KS"] == 0 and t["target"] == 512, what
                            if t["path"] == 2:
                                assert K > 96 or (epi == 2 and (W % 4 != 0 or zw < 4)), what     # else a register kernel exists
                                assert t["nkc"] == 1 or t["tpb"] == 1, what      # a re-staged panel: one tile per block
                        seen.add((t["path"], t["MT"], t["LEFT"], t["KS"], min(t["nkc"], 2)))
                        tpbs.add((t["path"], t["tpb"]))
    assert {(0, mt, ks) for mt in (1, 2, 3) for ks in (9, 18, 24)} <= seen
    assert {(1, mt, left, ks, 1) for ks, pairs in _PW_REGA.items() for mt, left in pairs} <= seen, \
        {(1, mt, left, ks, 1) for ks, pairs in _PW_REGA.items() for mt, left in pairs} - seen
    assert {(2, mt, 0, 0, n) for mt in range(1, 7) for n in (1, 2)} <= seen and {(3, 1, 0, 0, 1), (3, 1, 0, 0, 2), (3, 2, 0, 0, 1), (3, 2, 0, 0, 2), (3, 3, 0, 0, 1)} <= seen
    assert {(p, n) for p in (0, 1, 2) for n in (1, 2, 8)} <= tpbs and targets == {512, 1024}


def test_pw_plan_wgrad_contract():
    """kind 1: blocks of a multiple of 128 pixels cover the plane exactly once, the tile blocks cover M and N, and the workspace
    the fields imply is cidnet_pw_wgrad_ws_floats"""
    from hvi_cidnet_amd import _lib
    ws = _lib.lib().raw("cidnet_pw_wgrad_ws_floats")
    pchs, tiles = set(), set()
    for M in (1, 5, 16, 17, 36, 48, 49, 95, 190, 382):
        for N in (1, 5, 16, 17, 36, 48, 72, 95, 190):
            for B in (1, 3, 8):
                for HW in (1, 12, 127, 128, 129, 512, 513, 1028, 3750, 15000, 20001, 40063, 60000, 240000):
                    rc, t = _pw_plan(1, B, M, N, HW)
                    what = (B, M, N, HW, t)
                    assert rc == 0, what
                    assert t["pch"] % 128 == 0 and 512 <= t["pch"] <= 4096, what
                    assert t["chunks"] * t["pch"] >= HW > (t["chunks"] - 1) * t["pch"], what
                    assert t["last"] == HW - (t["chunks"] - 1) * t["pch"] and 1 <= t["last"] <= t["pch"], what
                    assert 1 <= t["MT"] <= 3 and 1 <= t["NT"] <= 3, what
                    assert t["nmb"] * 16 * t["MT"] >= M > (t["nmb"] - 1) * 16 * t["MT"] - 15, what
                    assert t["nnb"] * 16 * t["NT"] >= N > (t["nnb"] - 1) * 16 * t["NT"] - 15, what
                    assert t["n_red"] == B * t["chunks"] and t["n_red_ps"] == t["chunks"], what
                    assert ws(B, M, N, HW) == B * t["chunks"] * M * N, what
                    pchs.add(t["pch"])
                    tiles.add((t["MT"], t["NT"]))
    assert tiles == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)} and len(pchs) >= 4 and 512 in pchs


def test_pw_plan_bf16x3_and_fused_contract():
    """kinds 2 and 3: the waves' tiles cover M with at most five per wave, the prepared-weight workspace the fields imply is
    cidnet_pw_conv_bf16x3_ws_floats, the fused backward's persistent grid never exceeds 512 blocks and its rounds cover every
    chunk, and the shape error agrees with the *_supported predicates"""
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    ws = L.raw("cidnet_pw_conv_bf16x3_ws_floats")
    layouts, cpgs = set(), set()
    for M in (1, 16, 17, 32, 33, 36, 64, 80, 81, 96, 160, 161, 190, 320, 321, 336, 640, 766):
        for K in (1, 23, 24, 25, 33, 36, 48, 49, 72, 95, 144, 766):
            for HW in (1, 63, 64, 65, 127, 128, 130, 256, 257, 3750, 60000):
                rc, t = _pw_plan(2, 2, M, K, HW)
                what = (M, K, HW, t)
                assert rc == (0 if L.raw("cidnet_pw_conv_bf16x3_supported")(M, K, HW) else -2), what
                if rc:
                    continue
                assert t["cpg"] in (6, 8) and t["KB"] * 4 * t["cpg"] >= K > (t["KB"] - 1) * 4 * t["cpg"], what
                assert t["cpg"] == 8 or -(-K // 24) == -(-K // 32), what       # 24-channel k-blocks only where they cost none
                assert t["MT"] == -(-M // 16) and t["WM"] in (1, 2, 4) and 1 <= t["MTW"] <= 5, what
                assert t["WM"] * t["chunks"] * t["MTW"] * 16 >= M, what
                assert t["WM"] * t["chunks"] * (t["MTW"] - 1) < t["MT"], what   # no wave layer could go
                px = (4 // t["WM"]) * 64
                assert t["tiles"] * px >= HW > (t["tiles"] - 1) * px, what
                for B, ps in ((1, 0), (3, 0), (3, 1)):
                    assert ws(B, M, K, ps) == (B if ps else 1) * t["KB"] * t["MT"] * 3 * 256, what
                layouts.add((t["WM"], t["MTW"], t["chunks"]))
                cpgs.add(t["cpg"])
    assert {(1, 2, 1), (1, 5, 1), (2, 3, 1), (2, 5, 1), (4, 3, 1), (4, 5, 1), (4, 3, 2), (4, 5, 2)} <= layouts and cpgs == {6, 8}
    walks = set()
    for M, N in ((190, 36), (181, 33), (36, 95), (36, 36), (72, 36), (36, 72), (190, 72), (16, 36), (96, 36)):
        for B in (1, 2, 3, 8):
            for HW in (1, 3, 4, 6, 32, 36, 260, 5508, 16384, 16420, 60000):
                rc, t = _pw_plan(3, B, M, N, HW)
                what = (B, M, N, HW, t)
                assert rc == (0 if L.raw("cidnet_pw_bwd_fused_supported")(M, N, HW) else -2), what
                if rc:
                    assert L.raw("cidnet_pw_bwd_fused_ws_floats")(B, M, N, HW) == 0, what
                    continue
                assert (t["MT"], t["NT"]) == (-(-M // 16), -(-N // 16)), what
                assert t["chunks"] * 32 >= HW > (t["chunks"] - 1) * 32, what
                total = B * t["chunks"]
                assert 1 <= t["blocks"] == min(total, 512), what
                assert t["blocks"] * t["most"] >= total > t["blocks"] * (t["most"] - 1), what
                kb = (t["MT"] + 1) // 2
                assert L.raw("cidnet_pw_bwd_fused_ws_floats")(B, M, N, HW) == t["NT"] * kb * 3 * 256 + t["blocks"] * M * N, what
                walks.add(min(t["most"], 3))
    assert walks == {1, 2, 3}


def test_pw_plan_bad_arguments():
    from hvi_cidnet_amd import _lib
    q = _lib.lib().raw("cidnet_pw_plan")
    out = (ctypes.c_int * 14)()
    ok = (1, 36, 36, 1028, 0, 0, 0, 0, 0)
    assert q(0, *ok, out, 14) == 0
    for bad in ((-1, *ok), (4, *ok), (0, 0, 36, 36, 1028, 0, 0, 0, 0, 0), (0, 1, 0, 36, 1028, 0, 0, 0, 0, 0), (1, 1, 36, -1, 1028, 0, 0, 0, 0, 0),
                (2, 1, 36, 36, 0, 0, 0, 0, 0, 0), (0, 1, 36, 36, 1028, 0, 0, 2, 0, 0), (0, 1, 36, 36, 1028, 0, 0, 0, -1, 0),
                (0, 1, 36, 36, 1028, 0, 0, 0, 0, 3), (0, 1, 36, 36, 1028, 0, 0, 0, 0, -1),
                (0, 1, 36, 36, 1024, 16, 0, 0, 0, 2), (0, 1, 36, 36, 1024, 12, 8, 0, 0, 2), (0, 1, 36, 36, 1028, 16, 8, 0, 0, 2)):
        assert q(*bad, out, 14) == -1, bad
    assert q(0, 1, 36, 36, 1024, 16, 8, 0, 0, 2, out, 14) == 0
    assert q(0, *ok, None, 14) == -1
    for bad in ((0, 1, 36, 36, 1028, 0, 0, 1, 1, 0), (0, 1, 36, 36, 1024, 16, 8, 1, 0, 2), (0, 1, 36, 36, 1024, 16, 8, 0, 1, 2),
                (2, 1, 16, 36, 1028, 0, 0, 0, 0, 0), (3, 1, 36, 36, 1026, 0, 0, 0, 0, 0), (3, 1, 40, 100, 1028, 0, 0, 0, 0, 0)):
        assert q(*bad, out, 14) == -2, bad
    for kind, n in enumerate((14, 9, 7, 5)):
        assert q(kind, *ok, out, n) == 0 and q(kind, *ok, out, n - 1) == -1, kind


def test_product_path_refuses_cpu_tensors():
    import torch
    from hvi_cidnet_amd.hvi_transform import RGB_HVI
    m = RGB_HVI()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.HVIT(torch.rand(1, 3, 4, 4))


def test_product_package_does_not_import_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "hvi-cidnet_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_library_passes_the_code_object_checks():
    """The shipped code objects contain no v_pk_{fma,mul,add}_f32 and no SDWA instruction (hvi-cidnet_amd/build.py): beside
    LDS-fed bf16 MFMAs (csrc/conv3x.hip runs on both branch streams) packed-fp32 ops with op_sel in a neighbouring
    kernel's waves were seen to drop products (tools/mfma_pk_probe.hip).  And csrc/conv3xw.hip
    issues its staging loads as inline assembly: on every path from such a load to the wait that retires it no instruction
    may touch a destination register.  Both checks live in hvi-cidnet_amd/codeobj_check.py, which build.py also runs after
    linking; llvm-objdump is part of the image here and on the GPU box, so its absence is a failure, not a skip."""
    from hvi_cidnet_amd import _lib, codeobj_check
    assert os.path.exists(codeobj_check.OBJDUMP), codeobj_check.OBJDUMP
    bad, facts = codeobj_check.check_library(_lib.LIB_PATH)
    assert not bad, bad
    assert facts["code_objects"] >= 15 and facts["bf16_mfma"] > 0 and facts["asm_loads_checked"] >= 8, facts


def test_code_object_checker_sees_a_planted_hazard(tmp_path):
    """the data-flow pass finds a read of a load destination planted right after the barrier that follows the loads"""
    import re
    from hvi_cidnet_amd import _lib, codeobj_check
    found = False
    for co in codeobj_check.extract_code_objects(_lib.LIB_PATH, str(tmp_path)):
        dis = codeobj_check.disassemble(co, symbolize=True)
        if "conv3xw_kernel" not in dis:
            continue
        found = True
        h = codeobj_check._hazard_checker()
        names = codeobj_check.kernel_symbols(dis, "conv3xw_kernel")
        assert len(names) == 2                                      # operand levels 3 and 1
        lines = dis.splitlines()
        for name in names:
            assert not h.check(dis, name)[1]
            start = next(i for i, l in enumerate(lines) if l.rstrip().endswith(f"<{name}>:"))
            end = next((i for i in range(start + 1, len(lines)) if re.match(r"^[0-9a-f]+ <(?!L\d)", lines[i])), len(lines))
            # a copy of a load destination right after the barrier that follows the load: at least one load site of the
            # kernel is still pending there (the loads of the next tile cross the loop edge), and the pass must see it
            seen = False
            for site in (i for i in range(start, end) if "global_load_dwordx4" in lines[i]):
                reg = re.search(r"global_load_dwordx4 v\[(\d+):", lines[site]).group(1)
                bar = next((i for i in range(site, end) if "s_barrier" in lines[i]), None)
                if bar is None:
                    continue
                planted = lines[:bar + 1] + [f"\tv_mov_b32_e32 v250, v{reg}"] + lines[bar + 1:]
                seen = seen or bool(h.check("\n".join(planted), name)[1])
            assert seen, name
    assert found


def test_asm_load_hazard_checker_on_synthetic_assembly():
    """tools/asm_load_hazard.py models vmcnt as an in-order queue over the kernel's basic blocks: a read of a pending
    destination is found across a loop edge, a counted wait retires only the older loads, and clean code passes"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import asm_load_hazard as h
    finally:
        sys.path.pop(0)
    clean = """
k_kernel:
\tglobal_load_dwordx4 v[0:3], v[10:11], off
.LBB0_1:
\ts_waitcnt vmcnt(0)
\tv_add_f32_e32 v20, v0, v1
\tglobal_load_dwordx4 v[0:3], v[10:11], off
\ts_barrier
\ts_cbranch_scc1 .LBB0_1
\ts_waitcnt vmcnt(0)
\ts_endpgm
"""
    assert h.check(clean, "k_kernel") == (2, [])
    # a copy of the destination right after the barrier, i.e. before the wait at the loop top
    loop_edge = clean.replace("\ts_barrier\n", "\ts_barrier\n\tv_mov_b32_e32 v30, v2\n")
    assert h.check(loop_edge, "k_kernel")[1] == ["v_mov_b32_e32 v30, v2"]
    # vmcnt(1) retires the older of two loads only
    counted = """
k_kernel:
\tglobal_load_dwordx4 v[0:3], v[10:11], off
\tglobal_load_dwordx4 v[4:7], v[12:13], off
\ts_waitcnt vmcnt(1)
\tv_add_f32_e32 v20, v0, v1
\tv_add_f32_e32 v21, v4, v5
\ts_waitcnt vmcnt(0)
\ts_endpgm
"""
    assert h.check(counted, "k_kernel")[1] == ["v_add_f32_e32 v21, v4, v5"]
    # an address register that is itself a pending destination
    addr = counted.replace("\ts_waitcnt vmcnt(1)\n", "\tglobal_load_dwordx4 v[8:11], v[4:5], off\n\ts_waitcnt vmcnt(0)\n")
    assert h.check(addr, "k_kernel")[1] == ["global_load_dwordx4 v[8:11], v[4:5], off"]
