"""The host join of Havac::getDeviceWindowsFromFinishedRun (havac_windows_join: every chunk's and every GPU's sorted window list
joined again as weighted intervals) against havac.merge_windows over the union of the hits, and the new entry points exported by
the built libraries.  No device needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(windows):
    return [np.array([getattr(w, f) for w in windows], t) for f, t in
            (("sequenceIndex", np.uint32), ("phmmIndex", np.uint32), ("reverseStrand", np.uint8), ("sequenceStart", np.uint64),
             ("sequenceEnd", np.uint64), ("phmmFirst", np.uint32), ("phmmLast", np.uint32), ("hitCount", np.uint32))]


def join(lists):
    from havac_amd import _lib, havac
    flat = [w for lst in lists for w in lst]
    arrays = _arrays(flat)
    ends = np.cumsum([len(lst) for lst in lists]).astype(np.uint64)
    n = C.c_uint64(0)
    rc = _lib.load().havac_windows_join(len(flat), ends.ctypes.data, len(lists), *[a.ctypes.data for a in arrays], C.byref(n))
    assert rc == 0
    return havac._windows_from_arrays(arrays, n.value)


def random_hits(rng, nhits, record_lengths, model_lengths, cluster):
    from havac_amd import havac
    hits = []
    for _ in range(nhits):
        j = int(rng.integers(0, len(record_lengths)))
        k = int(rng.integers(0, len(model_lengths)))
        n = record_lengths[j]
        pos = int(rng.integers(0, min(n + 1, cluster))) if n else 0        # up to the terminator column
        hits.append(havac.HavacHit(pos, j, int(rng.integers(0, model_lengths[k] + 2)), k, bool(rng.integers(0, 2))))
    return hits


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("parts", [1, 2, 3, 7, 40])
def test_joined_lists_equal_one_merge_over_the_union(seed, parts):
    from havac_amd import havac
    rng = np.random.default_rng(seed)
    record_lengths = [int(v) for v in rng.integers(0, 3000, size=4)] + [0]
    model_lengths = [int(v) for v in rng.integers(1, 200, size=3)] + [0]
    hits = random_hits(rng, 1500, record_lengths, model_lengths, cluster=[300, 3000, 100000][seed % 3])
    for flank in (0, 1, 20, 1 << 30):
        want = havac.merge_windows(hits, model_lengths, record_lengths, flank)
        cut = np.sort(rng.integers(0, len(hits), size=parts - 1))
        pieces = np.split(np.arange(len(hits)), cut)
        lists = [havac.merge_windows([hits[i] for i in p], model_lengths, record_lengths, flank) for p in pieces]
        assert join(lists) == want, (seed, parts, flank)


def test_join_of_nothing_and_of_one_list():
    from havac_amd import havac
    assert join([]) == []
    assert join([[], []]) == []
    w = [havac.HavacWindow(0, 1, False, 5, 9, 2, 3, 4), havac.HavacWindow(0, 1, True, 0, 2, 0, 0, 1)]
    assert join([w]) == w


def test_join_rejects_lists_that_do_not_add_up():
    from havac_amd import _lib
    arrays = _arrays([])
    ends = np.array([3], np.uint64)
    n = C.c_uint64(0)
    assert _lib.load().havac_windows_join(2, ends.ctypes.data, 1, *[None] * 8, C.byref(n)) < 0
    assert _lib.load().havac_windows_join(0, ends.ctypes.data, 1, *[a.ctypes.data for a in arrays], C.byref(n)) < 0


def test_new_symbols_are_exported():
    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "havac_amd", lib)], capture_output=True, text=True,
                             check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    dev = exported("libhavac_dev.so")
    for name in ("havac_dev_compute_windows", "havac_dev_read_windows", "havac_dev_set_window_chunk", "havac_dev_window_stats",
                 "havac_windows_join"):
        assert name in dev, name
    host = exported("libhavac.so")
    for name in ("havac_host_get_device_windows", "havac_host_set_window_chunk", "havac_host_window_scratch_bytes",
                 "havac_host_windows_of_records"):
        assert name in host, name
    from havac_amd import _lib, havac
    _lib.load()
    havac.load_host()                       # every signature binds


def test_host_path_on_explicit_tables_equals_the_checker():
    """havac_host_windows_of_records (the host path after its read-back, used to time it against the device path) against the
    numpy resolver and merge_windows"""
    from havac_amd import havac, synth
    from oracle.resolve import expected_hits
    rng = np.random.default_rng(4)
    lengths = np.array([3000, 0, 17, 40000], np.int64)
    models = np.array([50, 300, 7], np.uint32)
    ends = np.cumsum(lengths + 1).astype(np.uint64)
    cols = np.sort(rng.integers(0, 2 * synth.SEGMENT * 2, size=5000)).astype(np.uint64)          # includes padding columns
    rows = rng.integers(0, int(models.sum()), size=cols.size).astype(np.uint64)
    seg, inseg = cols // np.uint64(synth.SEGMENT), cols % np.uint64(synth.SEGMENT)
    raw = np.ascontiguousarray((rows << np.uint64(40)) | (seg << np.uint64(14)) | inseg, np.uint64)
    arrays = [np.empty(raw.size, t) for t in (np.uint32, np.uint32, np.uint8, np.uint64, np.uint64, np.uint32, np.uint32, np.uint32)]
    n = C.c_uint32(0)
    for flank in (0, 20):
        rc = havac.load_host().havac_host_windows_of_records(raw.ctypes.data, raw.size, ends.ctypes.data, ends.size, models.ctypes.data,
                                                             models.size, flank, *[a.ctypes.data for a in arrays], raw.size, C.byref(n))
        assert rc == 0
        hits = [havac.HavacHit(*h) for h in expected_hits(raw, lengths, models)]
        assert havac._windows_from_arrays(arrays, n.value) == havac.merge_windows(hits, models.tolist(), lengths.tolist(), flank)
