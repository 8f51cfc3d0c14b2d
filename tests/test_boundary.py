"""The drop-in boundary without a GPU: the C-ABI libraries load, export every symbol the headers
declare, refuse to work without a device (no CPU fallback), and the product never touches oracle/."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from havac_amd import _lib, havac


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(havac_[a-z0-9_]+)\s*\(", text)))


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_device_library_exports_everything_in_havac_dev_h():
    names = declared_functions("havac_dev.h")
    assert len(names) >= 20
    have = exported(_lib.LIB_PATH)
    assert not [n for n in names if n not in have]
    assert sorted(_lib.SIGNATURES) == names            # the ctypes table covers the header, no more, no less
    assert b"gfx950" in _lib.load().havac_dev_version()


def test_host_library_exports_everything_in_havac_host_h():
    names = declared_functions("havac_host.h")
    have = exported(havac.HOST_LIB_PATH)
    assert not [n for n in names if n not in have]
    assert sorted(havac.HOST_SIGNATURES) == names
    havac.load_host()


def test_cpp_api_symbols_present():
    """The C++ class keeps the reference's method names (host/Havac.hpp:42-107)."""
    out = subprocess.run(["nm", "-DC", "--defined-only", havac.HOST_LIB_PATH], capture_output=True, text=True, check=True).stdout
    for method in ("Havac::loadSequence", "Havac::loadPhmm", "Havac::runHardwareClient()", "Havac::runHardwareClientAsync",
                   "Havac::waitHardwareClientAsync", "Havac::abortHardwareClient", "Havac::getHitsFromFinishedRun",
                   "Havac::currentHardwareState", "HavacHit::toString", "SequencePreprocessor::SequencePreprocessor",
                   "PhmmPreprocessor::PhmmPreprocessor", "p7HmmProjectForThreshold256", "findThreshold256ScalingFactor",
                   "esl_gumbel_invsurv", "phmmPrefixSumsBinarySearch"):
        assert method in out, method


def test_code_object_is_gfx950_only():
    """One offload bundle entry, for gfx950 (rocprim's host-side arch-name table is not a code object)."""
    strings = subprocess.run(["strings", "-n", "6", _lib.LIB_PATH], capture_output=True, text=True).stdout
    targets = set(re.findall(r"hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", strings))
    assert targets == {"gfx950"}
    assert "nvptx" not in strings and "sm_90" not in strings


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback_without_a_device():
    L = _lib.load()
    h = C.c_void_p()
    assert L.havac_dev_create(0, C.byref(h)) == _lib.E_NO_DEVICE
    assert L.havac_ssv_ctx_create(C.byref(h)) == _lib.E_NO_DEVICE
    from havac_amd.hw_client import HavacHwClient, NoDeviceError
    with pytest.raises(NoDeviceError):
        HavacHwClient()
    with pytest.raises(NoDeviceError):
        havac.Havac()


def test_product_never_touches_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "havac_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".h", ".hip", ".sh")):
                text = open(os.path.join(base, f), errors="ignore").read()
                if re.search(r"(?m)^\s*(from|import)\s+oracle\b|pyoracle|liboracle|ssv_oracle|softssv_ref|refhost|ssv_ref2", text):
                    bad.append(os.path.join(base, f))
    assert not bad
    for lib in (_lib.LIB_PATH, havac.HOST_LIB_PATH):
        needed = subprocess.run(["readelf", "-d", lib], capture_output=True, text=True).stdout
        assert "oracle" not in needed and "softssv" not in needed and "refhost" not in needed
    bench = open(os.path.join(ROOT, "bench.py")).read()
    assert "refhost" not in bench and "_ref2" not in bench


REFERENCE_HOST = "/root/reference/host/Havac.cpp"
REFHOST_LIB = os.path.join(ROOT, "oracle", "_ref", "libhavac_refhost.so")


@pytest.mark.skipif(not (os.path.isfile(REFERENCE_HOST) or os.path.isfile(REFHOST_LIB)),
                    reason="oracle/_ref/libhavac_refhost.so was not built (that needs the reference tree)")
def test_reference_host_code_compiles_against_the_committed_binding():
    """INTEGRATION.md section B as a build, not as prose: host/Havac.cpp, host/phmm/PhmmPreprocessor.cpp,
    host/sequence/SequencePreprocessor.cpp and PhmmReprojection/PhmmReprojection.cpp of the reference compile UNCHANGED,
    from where they lie, against integration/HavacHwClient.hpp + include/havac_dev.h (oracle/refhost.mk), and the
    result links to libhavac_dev.so alone.  Round 2's shim lived in a markdown block, lacked <iostream>, and did not
    compile; this test is what keeps that from happening again."""
    from refhost import binding
    assert binding.build_if_possible()
    have = subprocess.run(["nm", "-DC", "--defined-only", binding.REFHOST_LIB], capture_output=True, text=True, check=True).stdout
    for symbol in ("Havac::loadPhmm", "Havac::loadSequence", "Havac::runHardwareClientAsync", "Havac::getHitsFromFinishedRun",
                   "Havac::generatePhmmLenPrefixSums", "SequencePreprocessor::getCompressedSymbol",
                   "PhmmPreprocessor::getProcessedPhmmData", "p7HmmProjectForThreshold256", "HavacHwClient::getHitList"):
        assert symbol in have, symbol
    needed = subprocess.run(["readelf", "-d", binding.REFHOST_LIB], capture_output=True, text=True).stdout
    assert "libhavac_dev.so" in needed and "libhavac.so" not in needed and "xrt" not in needed
    # the markdown points at the committed header; it carries declarations only, no second implementation to go stale
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "integration/HavacHwClient.hpp" in doc and "havac_dev_destroy(dev)" not in doc
    assert os.path.isfile(binding.SSV_REF2_LIB)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_reference_havac_refuses_to_start_without_a_device():
    """The reference's constructor (host/Havac.cpp:20-31) over the binding: no device -> std::runtime_error out of
    make_shared<HavacHwClient>, nothing is computed anywhere else."""
    from refhost import binding
    if not os.path.isfile(binding.REFHOST_LIB):
        pytest.skip("oracle/_ref/libhavac_refhost.so was not built")
    with pytest.raises(binding.RefHostError) as e:
        binding.ReferenceHavac(0, 0.02)
    assert e.value.code == -3


def test_shard_arithmetic_is_host_only():
    """havac_ssv_shard_columns / shard_cells need no device: shards are runs of whole segments that tile the columns."""
    from havac_amd.ssv import shard_cells, shard_columns
    n, rows = 41 * 12288, 1000
    for world in (1, 2, 3, 8, 41):
        spans = [shard_columns(n, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
        assert all(b % 12288 == 0 and e % 12288 == 0 and e > b for b, e in spans)
        assert sum(shard_cells(n, rows, r, world) for r in range(world)) == n * rows
        widths = [e - b for b, e in spans]
        assert max(widths) - min(widths) <= 12288


def test_shard_windows_are_host_only_arithmetic():
    """havac_ssv_shard_window: whole segments, clipped to the database, containing the shard's own columns and a left
    halo of at least rows - 1 columns."""
    from havac_amd.ssv import shard_columns, shard_window
    n = 900 * 12288
    for rows in (1, 1024, 20000, 503329):
        for world in (1, 2, 8):
            for r in range(world):
                lo, hi = shard_columns(n, r, world)
                first, end = shard_window(n, rows, r, world)
                assert first % 12288 == 0 and end % 12288 == 0 and 0 <= first <= lo and hi <= end <= n
                assert first == 0 or lo - first >= rows - 1
                assert lo - first <= rows + 32 + 4096 + 12288 and end - hi <= 4096 + 12288


def test_ssv_kernel_resources():
    """What the hot kernel's speed rests on, read from the metadata of the code object inside libhavac_dev.so: 80 VGPRs
    (= six waves per SIMD), no scratch, no register spills, 14 KB of LDS per workgroup.  A change
    that costs a wave per SIMD costs 3 % and is easy to miss on a GPU box; here it fails on the CPU."""
    import re
    import shutil
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not all(os.path.isfile(os.path.join(llvm, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm's LLVM tools are not installed here")
    lib = os.path.join(ROOT, "havac_amd", "libhavac_dev.so")
    tmp = tempfile.mkdtemp(prefix="havac_co_")
    try:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.hsaco")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        symbols = subprocess.run([os.path.join(llvm, "llvm-readelf"), "-s", co], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|"
                                                         r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    hot = [v for k, v in kernels.items() if "15ssv_diag_kernel" in k]
    assert len(hot) == 1, sorted(kernels)
    hot = hot[0]
    assert hot["vgpr_count"] <= 80, hot                      # 512 / 6 in granules of 8: six waves per SIMD
    assert hot["private_segment_fixed_size"] == 0, hot       # no scratch
    assert hot["sgpr_spill_count"] == 0 and hot["vgpr_spill_count"] == 0, hot
    assert hot["group_segment_fixed_size"] <= 160 * 1024 // 6, hot      # six workgroups per CU fit the LDS
    # the resident-table kernel for short models (round 4): the same windows, six waves per SIMD too, no scratch either; its nine
    # tables (25 KB per workgroup) leave room for six workgroups per CU
    short = [v for k, v in kernels.items() if "19ssv_resident_kernel" in k]
    assert len(short) == 1, sorted(kernels)
    short = short[0]
    assert short["vgpr_count"] <= 80, short
    assert short["private_segment_fixed_size"] == 0 and short["sgpr_spill_count"] == 0 and short["vgpr_spill_count"] == 0, short
    assert short["group_segment_fixed_size"] <= 160 * 1024 // 6, short
    # ... and its instantiation for launches with a separator mask (round 5: ssv_resident_kernel_masked): the same budget
    masked = [v for k, v in kernels.items() if "26ssv_resident_kernel_masked" in k]
    assert len(masked) == 1, sorted(kernels)
    masked = masked[0]
    assert masked["vgpr_count"] <= 80 and masked["private_segment_fixed_size"] == 0 and masked["vgpr_spill_count"] == 0 and masked["sgpr_spill_count"] == 0, masked
    assert masked["group_segment_fixed_size"] <= 160 * 1024 // 6, masked
    assert any("ssv_diag_kernel_traced" in k for k in kernels) and any("ssv_gather_tails" in k for k in kernels)
    # The ordering kernels of passes that run beside each other (hit_order.hip.h) fit into the 32 VGPRs the SSV kernel leaves free
    # on a SIMD (512 - 6 x 80): a pass's ordering then runs in the shadow of the next pass's kernel instead of displacing its
    # waves.  (What does not fit -- three loop invariants of the in-register sorter -- is parked in scratch.)
    for name, scratch in (("ssv_order_count", 0), ("ssv_order_scatter", 0), ("ssv_order_sortE", 32), ("ssv_order_finish", 0)):
        k = [v for key, v in kernels.items() if name in key]
        assert len(k) == 1 and k[0]["vgpr_count"] <= 32 and k[0]["private_segment_fixed_size"] <= scratch, (name, k)
    assert len([v for key, v in kernels.items() if "ssv_order_scan" in key]) == 1
    # The kernel body reads rarely used arguments from the kernarg segment (rare_args); inside a function that is really CALLED
    # the pointer to that segment is null.  Only these two device functions may exist as functions of their own -- both are
    # handed what they need -- and in particular no outlined piece of the kernel body (its item lambda).
    functions = {line.split()[-1] for line in symbols.splitlines() if " FUNC " in line and "havac" in line}
    callees = {f for f in functions if not re.match(r"^_ZN5havac\d+ssv_[a-z_]+E", f)}      # the kernels are havac::ssv_*
    assert all(("flush_full" in f) or ("trace_cells_of_step" in f) for f in callees), sorted(callees)


def _device_isa(tmpdir):
    """the gfx950 ISA of havac_dev.hip with the compiler's block names kept (what tools/asm_chunk.py finds its regions by):
    a device-only compile, ~12 s"""
    import subprocess
    out = os.path.join(tmpdir, "havac_dev.s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-fno-discard-value-names", "-S",
                    "-o", out, os.path.join(ROOT, "havac_amd", "csrc", "havac_dev.hip")], check=True, capture_output=True, cwd=tmpdir)
    return out


def test_ssv_kernel_instruction_mix(tmp_path):
    """The hot loop's instruction mix, asserted from the disassembly (the register allocation at exactly
    80 VGPRs is one unrelated edit away from breaking, and VGPR count / scratch alone do not show a loop that got longer).
    One 32-step chunk on its usual path -- no matrix edge, four-step windows, no hit -- is 16 registers x 32 steps = 512
    `v_pk_add_i16 ... clamp` and at most 628 vector instructions in all (72 for the hit tests, 15
    window expansions, 5 `v_perm` + a handful for the tables); 256 `ds_read_b64` in the windows; nothing from scratch."""
    import importlib.util
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not installed here")
    spec = importlib.util.spec_from_file_location("asm_chunk", os.path.join(ROOT, "tools", "asm_chunk.py"))
    asm_chunk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(asm_chunk)
    isa = _device_isa(str(tmp_path))
    mix = asm_chunk.chunk_mix(isa, "_ZN5havac15ssv_diag_kernel")
    chunk, windows = mix["chunk"], mix["windows"]
    valu = asm_chunk.total(chunk, ("v_",))
    assert chunk["v_pk_add_i16"] == 512, dict(chunk)
    assert valu <= 628, (valu, {k: n for k, n in chunk.items() if k.startswith("v_")})      # (619 + the 8 moves of the window's slide, counted since round 4)
    assert windows["ds_read_b64"] == 256, dict(windows)
    assert asm_chunk.total(chunk, ("scratch_",)) == 0 and asm_chunk.total(chunk, ("v_readlane", "v_writelane")) == 0, dict(chunk)
    # the hit test: one OR tree + one compare per four-step window, on the vector unit; everything else of a window is adds
    assert chunk["v_or3_b32"] + chunk["v_bitop3_b32"] + chunk["v_cmp_ne_u32_e64"] <= 72, dict(chunk)
    # the resident-table kernel runs the same windows and builds no table inside a chunk (its register allocation is as easy to
    # upset as the standard kernel's: a tile loop written without the lambda around a tile's body moved 130-160 registers per
    # chunk and spilled, at 30.5 instead of 39.8 TCUPS on 32 rows)
    short = asm_chunk.chunk_mix(isa, "_ZN5havac19ssv_resident_kernel")
    # (its chunk is two calls of four windows since round 5 -- the second is skipped where a short model ends in the chunk's first
    # half -- so the reads are counted over the whole chunk, not over the region between the first and the last window)
    assert short["chunk"]["v_pk_add_i16"] == 512 and short["chunk"]["ds_read_b64"] == 256, dict(short["chunk"])
    assert asm_chunk.total(short["chunk"], ("v_",)) <= 625 and asm_chunk.total(short["chunk"], ("scratch_",)) == 0, dict(short["chunk"])
    assert short["chunk"].get("v_perm_b32", 0) == 0 and asm_chunk.total(short["chunk"], ("ds_write",)) == 0, dict(short["chunk"])
