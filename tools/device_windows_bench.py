"""Times a finished run's windows two ways on the same run, on bench.py's own inputs (bench.make_inputs) through a one-GPU handle of
the device layer:

  host path    havac_dev_read_hits64 (the whole record list to host memory) + havac_host_windows_of_records (Havac.hpp:
               havacWindowsOfRecords: the resolve, stretch, sort and merge Havac::getWindowsFromFinishedRun runs after its read-back)
  device path  havac_dev_compute_windows + havac_dev_read_windows (Havac::getDeviceWindowsFromFinishedRun's calls): merged on the
               GPU, only windows read back

Shapes (plain layout, one strand, one record over the real columns, the rest padding):
  c2        bench.py's C2: 1 model L=1024 x 100 Mbp (1.0e6 records)
  c3        bench.py's C3: the 1000-model collection (503,329 rows) x 10 Mbp
  c4shard   bench.py's C4 database (1 Gbp), the columns rank 5 of 8 owns (1.25e8), at full height (503,329 rows): the run of
            tests/test_gpu_scale.py's rank-5 case on a one-GPU handle.  Device path only by default: the host path needs ~80 B of
            host memory per record.

Each time is taken with the device synchronised before and after; the device path is timed on its second call (the first grows
its scratch).  Read-back bytes are what crossed PCIe: the records (8 B each) for the host path, every chunk's windows (40 B each,
before they are joined) for the device path.  One JSON line per shape.

    python tools/device_windows_bench.py --shapes c2 c3 c4shard --flank 20
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: the HIP runtime the libraries bind to)

import bench  # noqa: E402
from havac_amd import _lib, havac, synth  # noqa: E402
from havac_amd.hw_client import HavacHwClient  # noqa: E402

FIELDS = (np.uint32, np.uint32, np.uint8, np.uint64, np.uint64, np.uint32, np.uint32, np.uint32)


def inputs(shape):
    """-> (model table, packed sequence, real columns, model lengths)"""
    if shape == "c4shard":
        model, packed, ncols, _, _ = bench.make_inputs("c4", 8)
        b, e = C.c_uint64(0), C.c_uint64(0)
        assert _lib.load().havac_ssv_shard_columns(ncols, 5, 8, C.byref(b), C.byref(e)) == 0
        return model, np.ascontiguousarray(packed[b.value // 4: e.value // 4]), e.value - b.value, synth.model_lengths(1000)
    model, packed, ncols, _, _ = bench.make_inputs(shape, 1)
    real = bench.WORKLOADS[shape]["real"]
    lengths = [model.shape[0]] if bench.WORKLOADS[shape]["rows"] else synth.model_lengths(1000)
    return model, packed, real, lengths


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def device_path(c, ends, lens, flank):
    L = _lib.load()
    n = C.c_uint64(0)
    c._check(L.havac_dev_compute_windows(c._h, ends.ctypes.data, ends.size, lens.ctypes.data, lens.size, None, None, None, 0, flank,
                                         C.byref(n)))
    arrays = [np.empty(n.value, t) for t in FIELDS]
    got, at = C.c_uint64(0), 0
    while at < n.value:
        c._check(L.havac_dev_read_windows(c._h, min(1 << 20, n.value - at), *[a[at:].ctypes.data for a in arrays], C.byref(got)))
        at += got.value
    return arrays


def host_path(c, ends, lens, flank):
    raw = c.getHitList()
    arrays = [np.empty(raw.size, t) for t in FIELDS]            # (at most one window per record; untouched pages cost nothing)
    n = C.c_uint32(0)
    rc = havac.load_host().havac_host_windows_of_records(raw.ctypes.data, raw.size, ends.ctypes.data, ends.size, lens.ctypes.data,
                                                         lens.size, flank, *[a.ctypes.data for a in arrays], raw.size, C.byref(n))
    assert rc == 0, rc
    return [a[:n.value] for a in arrays], raw.size


def measure(shape, flank, host_shapes):
    model, packed, real, lengths = inputs(shape)
    ends = np.array([real], np.uint64)                           # one record of real - 1 residues (+ its terminator)
    lens = np.ascontiguousarray(lengths, np.uint32)
    assert int(lens.sum()) == model.shape[0]
    c = HavacHwClient(deviceIndex=0)
    try:
        c.setHitCapacity(1 << 30)
        c.writeSequence(packed)
        c.writePhmm(model)
        c.invokeHavacSsvAsync()
        _, run_ms = timed(lambda: c.waitForHavacSsvAsync())
        n64 = C.c_uint64(0)
        c._check(_lib.load().havac_dev_num_hits64(c._h, C.byref(n64)))
        device_path(c, ends, lens, flank + 1)
        dev, dev_ms = timed(lambda: device_path(c, ends, lens, flank))
        scratch, read_back = C.c_uint64(0), C.c_uint64(0)
        c._check(_lib.load().havac_dev_window_stats(c._h, C.byref(scratch), C.byref(read_back)))
        row = dict(shape=shape, flank=flank, records=n64.value, wait_ms=round(run_ms, 2), device_ms=round(dev_ms, 2),
                   windows=int(dev[0].size), hits_in_windows=int(dev[7].astype(np.uint64).sum()),
                   device_bytes_read_back=read_back.value, scratch_high_water_bytes=scratch.value,
                   host_max_rss_gb=round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20, 2))
        if shape in host_shapes:
            (host, nraw), host_ms = timed(lambda: host_path(c, ends, lens, flank))
            row.update(host_ms=round(host_ms, 2), host_windows=int(host[0].size), host_bytes_read_back=nraw * 8,
                       equal=all(np.array_equal(a, b) for a, b in zip(host, dev)))
        return row
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["c2", "c3"], choices=["c2", "c3", "c4shard"])
    ap.add_argument("--flank", type=int, default=20)
    ap.add_argument("--host-shapes", nargs="*", default=["c2", "c3"], help="shapes the host path is timed on as well")
    args = ap.parse_args()
    for shape in args.shapes:
        print(json.dumps(measure(shape, args.flank, args.host_shapes)), flush=True)


if __name__ == "__main__":
    main()
