"""A streamed search (Havac::searchFastaFile) against one load (loadSequence + runHardwareClient + getHitsFromFinishedRun) of
the same synthetic FASTA: wall time, peak host resident memory and the most text held, for each, and their hit counts, which
must be equal.  Each side runs in a fresh child process of its own, so that its peak RSS is its own; both go through the C ABI
(include/havac_host.h) and keep the same lists (hits and raw records), so no Python object per hit distorts either side.
    python tools/search_stream_bench.py [residues] [total_model_rows] [block_columns] [p_value]
defaults: 1 Gbp in 20 records, C3-like models (503,329 rows; lengths of a Dfam-like collection), the library's block size, and
a P-value of 1e-5: at bench.py's 0.02 C3's models find 4.5 hits per column of random sequence, 4.5e9 at 1 Gbp, more than one
pass's hit buffer holds; at 1e-5 about 2e6, so that what is measured is the database's way through the host and the device.
Prints one JSON line."""
import ctypes as C
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_inputs(d, n, rows):
    from havac_amd import synth
    fa, hmm = os.path.join(d, "db.fa"), os.path.join(d, "models.hmm")
    rng = np.random.default_rng(1)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    nrec, width = 20, 60
    with open(fa, "wb") as f:
        for k in range(nrec):
            m = n // nrec
            s = letters[rng.integers(0, 4, size=m, dtype=np.uint8)]
            s[rng.integers(0, m, size=64)] = ord("N")                # a few ambiguity codes: they draw from rand()
            pad = (-m) % width
            body = np.concatenate([s, np.full(pad, ord("A"), np.uint8)]).reshape(-1, width)
            lines = np.concatenate([body, np.full((body.shape[0], 1), ord("\n"), np.uint8)], axis=1)
            f.write(f">chr{k} synthetic\n".encode())
            f.write(lines.tobytes())
    models, total, k = [], 0, 0
    lengths = synth.model_lengths(2000)
    while total < rows:
        L = int(min(lengths[k % len(lengths)], rows - total)) or 1
        _, cons = synth.dfam_like_model(L, 500 + k)
        models.append(dict(name=f"fam{k}", acc=f"RF{k:05d}", emissions=synth.emissions_from_consensus(cons, 600 + k),
                           maxl=3 * L + 50, mu=-9.0, lam=0.71))
        total += L
        k += 1
    synth.write_hmm(hmm, models)
    return fa, hmm, len(models), total


def rss_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0      # (KiB on Linux)


def child(mode, fa, hmm, block_columns, p_value):
    from havac_amd import havac
    from havac_amd.hw_client import raise_for
    L = havac.load_host()
    h = C.c_void_p()
    raise_for(L.havac_host_create(0, p_value, C.byref(h)), "create")

    def ok(rc):
        if rc < 0:
            raise_for(rc, (L.havac_host_last_error(h) or b"").decode())

    ok(L.havac_host_load_phmm(h, os.fsencode(hmm)))
    C.CDLL(None).srand(1)
    before = rss_mb()
    n, nraw = C.c_uint32(0), C.c_uint64(0)
    t0 = time.perf_counter()
    if mode == "stream":
        ok(L.havac_host_search_fasta(h, os.fsencode(fa), block_columns, None, None))
        ok(L.havac_host_get_search_hits(h, None, None, None, None, None, 0, C.byref(n)))
        wall = time.perf_counter() - t0
        ok(L.havac_host_get_search_raw_hits(h, None, 0, C.byref(nraw)))
        raw = np.empty(nraw.value, np.uint64)
        ok(L.havac_host_get_search_raw_hits(h, raw.ctypes.data, raw.size, C.byref(nraw)))
        v = [C.c_uint64(0) for _ in range(4)]
        ok(L.havac_host_search_stats(h, *[C.byref(x) for x in v]))
        blocks, columns, _, text = (x.value for x in v)
    else:
        ok(L.havac_host_load_sequence(h, os.fsencode(fa)))
        ok(L.havac_host_run(h))
        ok(L.havac_host_get_hits(h, None, None, None, None, 0, C.byref(n)))
        wall = time.perf_counter() - t0
        r32 = C.c_uint32(0)
        ok(L.havac_host_get_raw_hits(h, None, 0, C.byref(r32)))
        raw = np.empty(r32.value, np.uint64)
        ok(L.havac_host_get_raw_hits(h, raw.ctypes.data, raw.size, C.byref(r32)))
        blocks, columns, text = 1, None, None                       # one load holds the whole text (FastaVector)
    out = dict(mode=mode, wall_s=round(wall, 3), peak_rss_mb=round(rss_mb(), 1), rss_before_mb=round(before, 1), hits=n.value,
               raw_records=int(raw.size), raw_xor=int(np.bitwise_xor.reduce(raw)) if raw.size else 0, blocks=blocks,
               reader_peak_bytes=text, columns=columns)
    L.havac_host_destroy(h)
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), float(sys.argv[6]))
        return
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 503_329
    block = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    p_value = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-5
    d = tempfile.mkdtemp(prefix="havac_stream_")
    t0 = time.time()
    fa, hmm, nmodels, total = write_inputs(d, n, rows)
    print(f"wrote {os.path.getsize(fa) / 1e6:.0f} MB FASTA and {nmodels} models / {total} rows in {time.time() - t0:.1f} s",
          file=sys.stderr, flush=True)
    res = {}
    for mode in ("stream", "load"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, fa, hmm, str(block), str(p_value)], capture_output=True,
                           text=True, timeout=1800)
        if r.returncode:
            print(r.stdout, r.stderr[-3000:], file=sys.stderr)
            raise SystemExit(f"{mode} child failed: rc {r.returncode}")
        res[mode] = json.loads(r.stdout.strip().splitlines()[-1])
        # a one-load text: what FastaVector holds -- the whole file's characters
        if mode == "load":
            res[mode]["reader_peak_bytes"] = res["stream"]["columns"]
    s, l = res["stream"], res["load"]
    line = dict(residues=n, model_rows=total, models=nmodels, block_columns=block or "default", p_value=p_value, stream=s, load=l,
                hits_equal=s["hits"] == l["hits"] and s["raw_xor"] == l["raw_xor"] and s["raw_records"] == l["raw_records"],
                wall_ratio=round(s["wall_s"] / l["wall_s"], 3), rss_ratio=round(s["peak_rss_mb"] / l["peak_rss_mb"], 3))
    for f in (fa, hmm):
        os.remove(f)
    os.rmdir(d)
    print(json.dumps(line), flush=True)
    if not line["hits_equal"]:
        raise SystemExit("the streamed search and one load found different hits")


if __name__ == "__main__":
    main()
