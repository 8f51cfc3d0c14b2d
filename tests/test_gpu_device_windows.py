"""Havac::getDeviceWindowsFromFinishedRun: a run's windows made on the GPU(s) that hold its records must equal, element for
element, what getWindowsFromFinishedRun gives on the host for the same run and flank, and what havac.merge_windows gives on the
CPU checker's records for that run's own inputs (resolved by oracle/resolve.py).  Every case runs with the default chunk and with a
chunk of a few hundred records, so that windows are joined across chunks."""
import ctypes as C
import os

import numpy as np
import pytest

from havac_amd import synth
from oracle.cases import boundary_raw, random_text, records_of, write_case
from oracle.resolve import expected_hits

pytestmark = pytest.mark.gpu

LIBC = C.CDLL(None)
TINY_CHUNK = 300
FLANKS = (0, 1, 20, 1 << 30)          # the last is larger than every record


def checker_windows(oracle, fa, hmm, flank, *, boundary=False, both=False, seed=0):
    """merge_windows over the CPU checker's records for these inputs (the product's layout, srand(seed) for the plain one)"""
    from havac_amd import havac
    if boundary:
        raw, lens = boundary_raw(fa, hmm, 0.02, oracle, both)
    else:
        packed, _, _ = havac.pack_fasta_layout(fa, False, both, seed=seed)
        table, lens = havac.project_hmm(hmm, 0.02)
        raw = oracle.ssv_fast(oracle.unpack_2bit(packed), table)
    lengths = [len(t) for t in records_of(fa)]
    hits = [havac.HavacHit(*h) for h in expected_hits(raw, lengths, lens, boundary=boundary, both_strands=both)]
    return havac.merge_windows(hits, lens, lengths, flank), raw


def open_handle(fa, hmm, *, boundary=False, both=False, seed=0, chunk=0, devices=None, depth=1):
    from havac_amd import havac
    h = havac.Havac(deviceIndices=devices) if devices else havac.Havac(0)
    h.setBoundaryMode(boundary)
    h.setBothStrands(both)
    h.setWindowChunk(chunk)
    if depth > 1:
        h.setPipelineDepth(depth)
    LIBC.srand(seed)
    h.loadSequence(fa)
    h.loadPhmm(hmm)
    return h


def check_case(oracle, fa, hmm, *, boundary=False, both=False, seed=0, min_windows=1):
    """one run per chunk setting; every flank: device windows == host windows (same run) == checker windows"""
    want = {f: checker_windows(oracle, fa, hmm, f, boundary=boundary, both=both, seed=seed) for f in FLANKS}
    for chunk in (0, TINY_CHUNK):
        h = open_handle(fa, hmm, boundary=boundary, both=both, seed=seed, chunk=chunk)
        try:
            h.runHardwareClient()
            for f in FLANKS:
                got = h.getDeviceWindowsFromFinishedRun(f)
                assert h.rawHits().size == 0                     # no record was read back
                host = h.getWindowsFromFinishedRun(f)
                assert np.array_equal(h.rawHits(), want[f][1])
                assert got == host, (chunk, f, len(got), len(host))
                assert got == want[f][0], (chunk, f)
            assert len(want[0][0]) >= min_windows
            assert h.getDeviceWindowsFromFinishedRun(0) == want[0][0]    # depth 1: the run stays current
        finally:
            h.close()
    return want


def test_plain_mode_models_records_padding_terminators_and_an_empty_record(tmp_path, oracle):
    rng = np.random.default_rng(3)
    # an A-only model hits poly-A text, the terminators and the A padding behind the last record; the other two are random
    # (twelve short poly-A records: terminators whose drawn symbol is A carry hits)
    texts = ["A" * 3000, ""] + ["A" * 200] * 12 + [random_text(5000, rng), "A" * 700 + random_text(900, rng)]
    fa, hmm = write_case(tmp_path, "plain", [40, 25, 90], texts, seed=1, consensus=0)
    want = check_case(oracle, fa, hmm, seed=11, min_windows=2)
    # the case holds what it is meant to: hits behind the last record, on terminator columns, on several models and records
    raw = want[0][1]
    lengths = [len(t) for t in records_of(fa)]
    cols = ((raw >> np.uint64(14)) & np.uint64(0x3FFFFFF)).astype(np.int64) * synth.SEGMENT + (raw & np.uint64(0x3FFF)).astype(np.int64)
    ends = np.cumsum(np.array(lengths) + 1)
    assert (cols >= ends[-1]).any() and np.isin(cols, ends - 1).any()
    assert len({(w.sequenceIndex, w.phmmIndex) for w in want[0][0]}) >= 3


def test_plain_mode_write_inputs(tmp_path, oracle):
    from test_gpu_api import write_inputs
    fa, hmm = write_inputs(tmp_path, [60, 300, 150], [5000, 9000, 30000, 17])
    check_case(oracle, fa, hmm, seed=4242, min_windows=3)


def test_boundary_mode(tmp_path, oracle):
    from test_gpu_api import write_inputs
    fa, hmm = write_inputs(tmp_path, [60, 300, 150], [5000, 9000, 30000, 17])
    check_case(oracle, fa, hmm, boundary=True, min_windows=3)


def test_both_strands(tmp_path, oracle):
    from test_gpu_api import write_inputs
    fa, hmm = write_inputs(tmp_path, [60, 300, 150], [5000, 9000, 30000, 17])
    want = check_case(oracle, fa, hmm, both=True, seed=77, min_windows=3)
    assert any(w.reverseStrand for w in want[0][0]) and any(not w.reverseStrand for w in want[0][0])


def test_both_strands_in_boundary_mode(tmp_path, oracle):
    from test_gpu_api import write_inputs
    fa, hmm = write_inputs(tmp_path, [60, 300, 150], [5000, 9000, 30000, 17])
    want = check_case(oracle, fa, hmm, boundary=True, both=True, min_windows=3)
    assert any(w.reverseStrand for w in want[0][0])


def test_a_run_with_no_hits(tmp_path, oracle):
    # a C-only model on G-only text: no three matching columns anywhere (the padding is A, a terminator one column)
    fa, hmm = write_case(tmp_path, "none", [30], ["G" * 5000, "G" * 300], consensus=1)
    want = check_case(oracle, fa, hmm, min_windows=0)
    assert want[0][1].size == 0 and want[0][0] == []


def test_dense_hits(tmp_path, oracle):
    # A-only models on poly-A text: nearly every cell past the first few of a diagonal is a hit (as fixture g5a's all-+127 model)
    fa, hmm = write_case(tmp_path, "dense", [24, 31], ["A" * 9000, "A" * 4000], consensus=0)
    want = check_case(oracle, fa, hmm, min_windows=2)
    assert want[0][1].size > 10_000


# ---- C2 through the device layer ------------------------------------------------------------------------------------------

def _device_windows(client, record_ends, model_lengths, flank, forward_columns=0):
    from havac_amd import _lib
    L = _lib.load()
    ends = np.ascontiguousarray(record_ends, np.uint64)
    lens = np.ascontiguousarray(model_lengths, np.uint32)
    n = C.c_uint64(0)
    client._check(L.havac_dev_compute_windows(client._h, ends.ctypes.data, ends.size, lens.ctypes.data, lens.size, None, None, None,
                                              forward_columns, flank, C.byref(n)))
    arrays = [np.empty(n.value, t) for t in (np.uint32, np.uint32, np.uint8, np.uint64, np.uint64, np.uint32, np.uint32, np.uint32)]
    got, at = C.c_uint64(0), 0
    while at < n.value:                                           # in slices: each read goes on where the last stopped
        take = min(100_000, n.value - at)
        client._check(L.havac_dev_read_windows(client._h, take, *[a[at:].ctypes.data for a in arrays], C.byref(got)))
        assert got.value == take
        at += take
    client._check(L.havac_dev_read_windows(client._h, 10, *[a.ctypes.data for a in arrays], C.byref(got)))
    assert got.value == 0                                         # all served
    return arrays


def test_c2_windows(oracle):
    """Config C2 as bench.py makes it (L=1024 x 100 Mbp, 1.0e6 records) on a handle of the device layer, split into three records
    and the padding: the windows equal merge_windows over the run's records resolved by the checker's resolver -- which is what
    getWindowsFromFinishedRun computes from the same list -- with the default chunk and with a chunk of a few hundred records."""
    import bench
    from havac_amd import havac
    from havac_amd.hw_client import HavacHwClient
    from havac_amd import _lib
    model, packed, ncols, _, _ = bench.make_inputs("c2", 1)
    lengths = np.array([40_000_000, 49, 60_000_000 - 60], np.int64)         # residues; the rest of the columns is padding
    ends = np.cumsum(lengths + 1).astype(np.uint64)
    c = HavacHwClient(deviceIndex=0)
    try:
        c.setHitCapacity(1 << 22)
        c.writeSequence(packed)
        c.writePhmm(model)
        c.invokeHavacSsvAsync()
        c.waitForHavacSsvAsync()
        raw = c.getHitList()
        assert raw.size > 1_000_000
        hits = [havac.HavacHit(*h) for h in expected_hits(raw, lengths, [model.shape[0]])]
        for flank in (0, 20):
            want = havac.merge_windows(hits, [model.shape[0]], lengths.tolist(), flank)
            for chunk in (0, TINY_CHUNK):
                c._check(_lib.load().havac_dev_set_window_chunk(c._h, chunk))
                si, pi, rs, st, en, pf, pl, hc = _device_windows(c, ends, [model.shape[0]], flank)
                assert si.size == len(want), (flank, chunk)
                assert np.array_equal(si, [w.sequenceIndex for w in want]) and np.array_equal(pi, [w.phmmIndex for w in want])
                assert not rs.any()
                assert np.array_equal(st, [w.sequenceStart for w in want]) and np.array_equal(en, [w.sequenceEnd for w in want])
                assert np.array_equal(pf, [w.phmmFirst for w in want]) and np.array_equal(pl, [w.phmmLast for w in want])
                assert np.array_equal(hc, [w.hitCount for w in want])
    finally:
        c.close()


# ---- runs in flight, failed runs, several parts, memory ------------------------------------------------------------------

def _inputs_of_three_runs(tmp_path):
    rng = np.random.default_rng(5)
    genome = rng.integers(0, 4, size=3000, dtype=np.uint8)
    texts = ["".join("ACGT"[v] for v in genome[:2500]) + random_text(4000, rng), random_text(3000, rng) + "".join("ACGT"[v] for v in genome[500:2900])]
    fa1, hmm1 = write_case(tmp_path, "r1", [60, 120], [texts[0]], seed=2)
    fa2, hmm2 = write_case(tmp_path, "r2", [200, 35, 80], [texts[1]], seed=3)
    # every model's consensus is a stretch of the genome the texts hold
    from havac_amd import synth as S
    for hmm, lens, off in ((hmm1, [60, 120], 100), (hmm2, [200, 35, 80], 700)):
        models = []
        for k, L in enumerate(lens):
            cons = genome[off + 300 * k:][:L]
            models.append(dict(name=f"m{k}", acc=f"RF{k:05d}", emissions=S.emissions_from_consensus(cons, 90 + k), maxl=3 * L + 50,
                               mu=-9.2 + 0.1 * k, lam=0.71))
        S.write_hmm(hmm, models)
    both = os.path.join(str(tmp_path), "r12.fa")
    with open(both, "w") as f:
        f.write(open(fa1).read() + open(fa2).read())
    return fa1, fa2, both, hmm1, hmm2


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("chunk", [0, TINY_CHUNK])
def test_runs_in_flight_each_resolved_against_its_own_inputs(tmp_path, oracle, depth, chunk):
    from havac_amd import havac
    fa1, fa2, fa12, hmm1, hmm2 = _inputs_of_three_runs(tmp_path)
    h = havac.Havac(0)
    try:
        h.setWindowChunk(chunk)
        h.setPipelineDepth(depth)
        LIBC.srand(1)
        h.loadSequence(fa1)
        h.loadPhmm(hmm1)
        runs = []
        h.runHardwareClientAsync(); runs.append((fa1, hmm1, 1))
        h.loadPhmm(hmm2)
        h.runHardwareClientAsync(); runs.append((fa1, hmm2, 1))
        LIBC.srand(2)
        h.loadSequence(fa2)                                   # appends: the run after this one has both files' records
        if depth == 2:                                        # (a slot for the third run)
            fa, hmm, seed = runs.pop(0)
            assert h.getDeviceWindowsFromFinishedRun(20) == checker_windows(oracle, fa, hmm, 20, seed=seed)[0]
        h.runHardwareClientAsync(); runs.append((fa12, hmm2, 2))
        for fa, hmm, seed in runs:
            want = checker_windows(oracle, fa, hmm, 20, seed=seed)[0]
            assert len(want) > 0
            assert h.getDeviceWindowsFromFinishedRun(20) == want, (fa, hmm)
        with pytest.raises(RuntimeError):
            h.getDeviceWindowsFromFinishedRun(0)              # no open run left
    finally:
        h.close()


def test_overflowed_run_raises_and_closes_it(tmp_path, oracle):
    from havac_amd import havac
    from havac_amd.hw_client import HitOverflowError
    from test_gpu_api import write_inputs
    fa, hmm = write_inputs(tmp_path, [60, 300, 150], [5000, 9000, 30000, 17])
    want, raw = checker_windows(oracle, fa, hmm, 3, seed=9)
    h = havac.Havac(0)
    try:
        h.setHitCapacity(max(1, raw.size // 2))
        h.setPipelineDepth(2)
        LIBC.srand(9)
        h.loadSequence(fa)
        h.loadPhmm(hmm)
        h.runHardwareClientAsync()
        h.runHardwareClientAsync()
        with pytest.raises(HitOverflowError):
            h.getDeviceWindowsFromFinishedRun(3)
        with pytest.raises(HitOverflowError):                 # the second run: the first was closed by the fetch that raised
            h.getDeviceWindowsFromFinishedRun(3)
        h.setHitCapacity(raw.size + 64)
        h.runHardwareClientAsync()
        assert h.getDeviceWindowsFromFinishedRun(3) == want
    finally:
        h.close()


def test_aborted_run_raises_logic_error_and_closes_it(tmp_path, oracle):
    """A long run (60,000 model rows x 2,000 segments) aborted at once, a short one behind it."""
    from havac_amd import havac
    from havac_amd.hw_client import LogicError
    rng = np.random.default_rng(8)
    fa_long, hmm_long = write_case(tmp_path, "long", [3000] * 20, [random_text(2000 * synth.SEGMENT - 100, rng)], seed=4)
    fa, hmm = write_case(tmp_path, "short", [50], ["A" * 4000], consensus=0)
    h = havac.Havac(0)
    try:
        h.setHitCapacity(1 << 24)
        h.setPipelineDepth(2)
        h.loadSequence(fa_long)
        h.loadPhmm(hmm_long)
        h.runHardwareClientAsync()
        h.abortHardwareClient()
        with pytest.raises(LogicError):
            h.getDeviceWindowsFromFinishedRun(0)
        h2 = open_handle(fa, hmm)
        try:
            h2.runHardwareClient()
            want = checker_windows(oracle, fa, hmm, 5)[0]
            assert h2.getDeviceWindowsFromFinishedRun(5) == want and len(want) > 0
        finally:
            h2.close()
        with pytest.raises(RuntimeError):
            h.getDeviceWindowsFromFinishedRun(0)              # the aborted run was closed: none is open
    finally:
        h.close()


@pytest.mark.parametrize("chunk", [0, TINY_CHUNK])
def test_three_parts_on_one_gpu_equal_one_part(tmp_path, oracle, chunk):
    """Records straddle the shard boundaries of a [0, 0, 0] handle (whole 12288-column segments per part)."""
    from test_gpu_api import write_inputs
    fa, hmm = write_inputs(tmp_path, [60, 300, 150], [20000, 15000, 9000, 17], seed=2)
    one = open_handle(fa, hmm, seed=6, chunk=chunk)
    three = open_handle(fa, hmm, seed=6, chunk=chunk, devices=[0, 0, 0])
    try:
        one.runHardwareClient()
        three.runHardwareClient()
        for f in (0, 20, 1 << 30):
            want = one.getWindowsFromFinishedRun(f)
            assert len(want) >= 3
            assert one.getDeviceWindowsFromFinishedRun(f) == want
            assert three.getDeviceWindowsFromFinishedRun(f) == want, f
        assert want == checker_windows(oracle, fa, hmm, 1 << 30, seed=6)[0]
    finally:
        one.close()
        three.close()


def test_device_memory_comes_back(tmp_path):
    import torch
    from test_gpu_api import write_inputs
    fa, hmm = write_inputs(tmp_path, [60, 300, 150], [50000, 9000, 30000, 17])
    dev = torch.device("cuda", 0)

    def cycle():
        h = open_handle(fa, hmm, seed=1, devices=[0, 0])
        try:
            h.runHardwareClient()
            for chunk in (0, TINY_CHUNK, 0):
                h.setWindowChunk(chunk)
                for f in (0, 20):
                    assert len(h.getDeviceWindowsFromFinishedRun(f)) > 0
            assert h.windowScratchBytes() > 0
        finally:
            h.close()
        torch.cuda.synchronize(dev)
        return torch.cuda.mem_get_info(dev)[0]

    start = cycle()
    for k in range(3):
        free = cycle()
        assert start - free < (64 << 20), f"cycle {k + 1}: {(start - free) / 2**20:.1f} MiB less free device memory"
