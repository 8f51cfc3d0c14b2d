"""One rank of tests/test_gpu_pipe_ranks.py: `python pipe_rank_worker.py RANK WORLD DIR MODE` (MODE: sync | stream).

Every rank shares GPU 0.  torch.distributed runs over gloo with a file store and carries only the communicator's id; the
records travel through libhavac_dev.so's own gather (havac_gather_*, the C route), which the pipe (havac_pipe.hip) drives
while later passes are in flight, bound to tests/native/librccl_standin.so.  MODE "stream" makes the stand-in enqueue its
operations as RCCL does (standin_set_stream_ordered) and puts a bounded kernel in front of each of them (standin_set_lag_ms):
a missing stream dependency in the pipe then shows up as a wrong list.  Each scenario writes what this rank saw into
DIR/result_RANK.json; every list is compared with the CPU checker here, element for element.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  -- first: see tests/conftest.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as tdist  # noqa: E402

from havac_amd import dist as D, synth  # noqa: E402
from havac_amd.hw_client import CollectiveTimeout, HitOverflowError  # noqa: E402
from havac_amd.ssv import shard_columns  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

STANDIN = os.path.join(ROOT, "tests", "native", "librccl_standin.so")
LAG_MS = 30                                                  # stream mode: the bounded kernel in front of every operation
CONFIGS = [(1, 1), (2, 1), (2, 2), (3, 2), (4, 3)]          # (depth, kernel streams)
SEG = synth.SEGMENT


def columns(records):
    r = records.view(np.uint64)
    return ((r >> np.uint64(14)) & np.uint64(0x3FFFFFF)) * np.uint64(SEG) + (r & np.uint64(0x3FFF))


def checker(sym, model):
    return O.ssv_fast(sym, model, nthreads=4)


def s1_inputs():
    """12 passes, each with its own seeded (sequence, model): heights on both sides of 256, 5 ... 12 segments; totals that rise
    over the first eight passes (every slot's receive buffer regrows at depth <= 4), pass 7 dense (a list of many mailbox
    chunks), pass 8 without a hit, pass 9 with hits only in the last sixth of the columns (the last rank's, at 2 and 3 ranks)"""
    heights = [96, 300, 180, 520, 240, 700, 128, 12, 260, 200, 333, 64]
    nsegs = [5, 6, 7, 8, 9, 10, 11, 12, 9, 12, 7, 6]
    passes, previous = [], 0
    for k in range(12):
        nrows, ncols = heights[k], nsegs[k] * SEG
        model, cons = synth.dfam_like_model(nrows, 500 + k)
        sym = synth.random_symbols(ncols, 600 + k)
        if k == 7:
            model = np.full((nrows, 4), 127, np.int8)            # a hit on every third row of every diagonal
        elif k == 8:
            model[model > 0] = 6                                  # no consensus run reaches 256
        elif k == 9:
            model[model > 0] = np.minimum(model[model > 0], 14)  # nothing in the random background ...
            tail = sym[ncols - ncols // 6:]                       # ... hits only where homologs are planted
            synth.plant_homologs(tail, cons, tail.size, every=3000, length=min(200, nrows), seed=700 + k)
        else:
            every = int(60000 / (k + 1) ** 1.6)
            while True:                                           # (rising totals, decided by the checker itself)
                trial = sym.copy()
                synth.plant_homologs(trial, cons, ncols, every=every, length=min(220, nrows), seed=700 + k)
                want = checker(trial, model)
                if k > 7 or want.size > previous * 1.2 + 16 or every < 400:
                    break
                every = int(every * 0.8)
            sym = trial
        want = checker(sym, model)
        previous = want.size
        passes.append((sym, model, want))
    return passes


def dense_pass(world):
    """a pass that overflows a small hit buffer only in the last rank's columns: a poly-A stretch in the last segment and a
    model that hits only on long runs of A"""
    nrows, ncols = 40, 8 * SEG
    sym = synth.random_symbols(ncols, 900)
    sym[ncols - SEG + 1000: ncols - SEG + 7000] = 0
    model = np.full((nrows, 4), -128, np.int8)
    model[:, 0] = 30
    return sym, model, checker(sym, model)


class Uploaded:
    """a pass's device inputs, kept alive until the pass is collected"""

    def __init__(self, dev, sym, model):
        self.seq = torch.from_numpy(synth.pack_2bit(sym)).to(dev)
        self.phmm = torch.from_numpy(np.ascontiguousarray(model).reshape(-1)).to(dev)
        self.n, self.rows = sym.size, model.shape[0]


def mine(want, n, rank, world):
    lo, hi = shard_columns(n, rank, world)
    c = columns(want)
    return int(((c >= lo) & (c < hi)).sum())


def run_s1(dev, rank, world, passes, uploads, depth, streams, capacity):
    """submit every pass, collect the oldest once every slot is in flight; rank 0 clones each list on the current stream at once
    (no host synchronise) and, at depth > 1, re-reads it just before its slot is submitted again"""
    eng = D.ShardedSsv(capacity, dev, depth=depth, kernel_streams=streams)
    out = {"c_route": bool(eng._c_route)}
    clones, rereads, returned, found = {}, {}, {}, {}
    order = []

    def collect():
        k = order.pop(0)
        merged, f = eng.collect()
        found[k] = f
        if rank == 0:
            clones[k] = merged.clone()
            returned[k] = merged
    for k, u in enumerate(uploads):
        if rank == 0 and depth > 1 and (k - depth) in returned:
            rereads[k - depth] = returned.pop(k - depth).clone()
        eng.submit(u.seq, u.n, u.phmm, u.rows, inputs_ready=True)
        order.append(k)
        if len(eng.in_flight) == depth:
            collect()
    while eng.in_flight:
        collect()
    eng.wait_gathers()
    torch.cuda.synchronize(dev)
    out["streams_used"] = eng.streams_used
    out["found_ok"] = [found[k] == mine(p[2], p[0].size, rank, world) for k, p in enumerate(passes)]
    if rank == 0:
        out["passes"] = len(clones)
        out["equal"] = [bool(np.array_equal(clones[k].cpu().numpy().view(np.uint64), p[2])) for k, p in enumerate(passes)]
        out["rereads"] = len(rereads)
        out["reread_equal"] = [bool(np.array_equal(v.cpu().numpy().view(np.uint64), passes[k][2])) for k, v in sorted(rereads.items())]
    eng.close()
    return out


def run_s2(dev, rank, world, passes, depth, streams):
    """good, good, overflowing (last rank only), good, good: two passes in flight on either side of the failed one"""
    sym_d, model_d, want_d = dense_pass(world)
    good = [passes[k] for k in (1, 2, 4, 6)]
    capacity = max(mine(p[2], p[0].size, r, world) for p in good for r in range(world)) + 64
    per_rank = [mine(want_d, sym_d.size, r, world) for r in range(world)]
    assert per_rank[-1] > capacity and max(per_rank[:-1]) <= capacity, (per_rank, capacity)
    seq = [good[0], good[1], (sym_d, model_d, want_d), good[2], good[3]]
    uploads = [Uploaded(dev, s, m) for s, m, _ in seq]
    torch.cuda.synchronize(dev)
    eng = D.ShardedSsv(capacity, dev, depth=depth, kernel_streams=streams)
    out = {"c_route": bool(eng._c_route), "lists": [], "found_ok": []}
    order = []

    def collect():
        k = order.pop(0)
        try:
            merged, f = eng.collect()
        except D.ShardFailure as e:
            out["failed"] = {"pass": k, "kind": "ShardFailure", "message": str(e)}
            return
        except HitOverflowError as e:
            out["failed"] = {"pass": k, "kind": "HitOverflowError", "message": str(e)}
            return
        out["found_ok"].append(f == mine(seq[k][2], seq[k][0].size, rank, world))
        if rank == 0:
            out["lists"].append(bool(np.array_equal(merged.clone().cpu().numpy().view(np.uint64), seq[k][2])))
    for k, u in enumerate(uploads):
        eng.submit(u.seq, u.n, u.phmm, u.rows, inputs_ready=True)
        order.append(k)
        if len(eng.in_flight) == depth:
            collect()
    while eng.in_flight:
        collect()
    eng.wait_gathers()
    torch.cuda.synchronize(dev)
    eng.close()
    return out


def run_s3(dev, rank, world, passes):
    """havac_pipe_run at (3, 2): two loops of different inputs; the last list of each equals the checker's"""
    eng = D.ShardedSsv(1 << 16, dev, depth=3, kernel_streams=2)
    out = {"c_route": bool(eng._c_route), "equal": [], "found_ok": []}
    for k in (5, 10):
        sym, model, want = passes[k]
        u = Uploaded(dev, sym, model)
        (merged, f), timings = eng.run_many(7, u.seq, u.n, u.phmm, u.rows)
        out["found_ok"].append(f == mine(want, sym.size, rank, world) and len(timings) == 7)
        if rank == 0:
            out["equal"].append(bool(np.array_equal(merged.clone().cpu().numpy().view(np.uint64), want)))
        eng.wait_gathers()
    torch.cuda.synchronize(dev)
    eng.close()
    return out


def run_s5(dev, rank, world, standin):
    """the stand-in really is asynchronous: right after havac_gather_records returns, rank 0's receive buffer, read through a
    stream that does not wait for the communicator's, still holds its pattern; after havac_gather_wait it holds the list"""
    g = D.c_gather(None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sizes = [5000 + 7000 * r for r in range(world)]
    data = [(np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(r) * np.uint64(1 << 40)) | np.uint64(1)
            for r, n in enumerate(sizes)]
    src = torch.from_numpy(data[rank].view(np.int64).copy()).to(dev)
    counts = g.counts(sizes[rank], stream)
    pattern = 0x5A5A5A5A5A5A5A5A
    dst = torch.full((sum(sizes),), pattern, dtype=torch.int64, device=dev) if rank == 0 else None
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)                  # (torch's pool streams are non-blocking: no implicit wait on anything)
    standin.standin_set_lag_ms(1000)
    t0 = time.time()
    g.records(src.data_ptr(), dst.data_ptr() if rank == 0 else 0, dst.numel() if rank == 0 else 0, stream)
    out = {"counts_ok": counts == sizes}
    if rank == 0:
        with torch.cuda.stream(side):
            early = dst.clone()
        side.synchronize()
        out["read_s"] = round(time.time() - t0, 3)
        out["pattern_before"] = bool((early.cpu() == pattern).all())
    standin.standin_set_lag_ms(LAG_MS)
    g.wait()
    torch.cuda.synchronize(dev)
    if rank == 0:
        out["list_after"] = bool(np.array_equal(dst.cpu().numpy().view(np.uint64), np.concatenate(data)))
    return out


def run_s4(dev, rank, world, passes, standin):
    """the records-stage deadline: a collect whose records are still behind a 1.5 s kernel, then wait_gathers() under 300 ms"""
    sym, model, _ = passes[3]
    u = Uploaded(dev, sym, model)
    torch.cuda.synchronize(dev)
    eng = D.ShardedSsv(1 << 16, dev, depth=2, kernel_streams=2)
    D.set_gather_deadline(0)
    standin.standin_set_lag_ms(1500)
    eng.submit(u.seq, u.n, u.phmm, u.rows, inputs_ready=True)
    eng.collect()                                  # (the count exchange waits the lag out, without a deadline)
    D.set_gather_deadline(0.3)
    t0 = time.time()
    try:
        eng.wait_gathers()
        out = {"message": "no error"}
    except CollectiveTimeout as e:
        out = {"message": str(e), "seconds": round(time.time() - t0, 2)}
    standin.standin_set_lag_ms(0)
    torch.cuda.synchronize(dev)                    # the bounded kernel ends by itself, and the records behind it move
    eng.close()
    D.close_c_gathers()                            # (the communicator is broken now: aborted)
    return out


def main():
    rank, world, directory, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tdist.init_process_group("gloo", init_method="file://" + os.path.join(directory, "store"), rank=rank, world_size=world)
    D.use_gather_library(STANDIN)
    standin = C.CDLL(STANDIN)                      # the same handle the library has bound
    standin.standin_set_lag_ms.argtypes = [C.c_uint32]
    standin.standin_set_stream_ordered.argtypes = [C.c_int]
    standin.standin_set_timeout_ms.argtypes = [C.c_uint32]
    standin.standin_set_timeout_ms(20000)          # (a lost message fails the run in 20 s, not 60)
    standin.standin_set_stream_ordered(1 if mode == "stream" else 0)
    standin.standin_set_lag_ms(LAG_MS if mode == "stream" else 0)
    out = {"rank": rank, "world": world, "mode": mode, "version": D.RcclGather.rccl_version(), "lag_ms": LAG_MS if mode == "stream" else 0}

    passes = s1_inputs()
    uploads = [Uploaded(dev, s, m) for s, m, _ in passes]
    torch.cuda.synchronize(dev)                    # (the inputs are in place: the passes are submitted with inputs_ready)
    capacity = max(mine(p[2], p[0].size, r, world) for p in passes for r in range(world)) + 1024
    out["s1"] = {f"{d},{s}": run_s1(dev, rank, world, passes, uploads, d, s, capacity) for d, s in CONFIGS}
    out["s2"] = {f"{d},{s}": run_s2(dev, rank, world, passes, d, s) for d, s in ((3, 2), (4, 3))}
    out["s3"] = run_s3(dev, rank, world, passes)
    if mode == "stream":
        out["s5"] = run_s5(dev, rank, world, standin)
        out["s4"] = run_s4(dev, rank, world, passes, standin)
    else:
        D.close_c_gathers()
    tdist.destroy_process_group()
    with open(os.path.join(directory, f"result_{rank}.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
