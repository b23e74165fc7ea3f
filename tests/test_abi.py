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
