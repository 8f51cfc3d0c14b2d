"""Inputs the tests of the hit resolver and of the run queue share: small FASTA / .hmm files with known edges, and the raw
records a run on them must give, found by the CPU checker on the product's own layouts (test infrastructure)."""
import os

import numpy as np

from havac_amd import synth

LUT_BOUNDARY = np.full(256, 3, np.uint8)            # host/test/Ssv.cpp:29-34: a/c/g as they are, everything else T
for _ch, _v in zip(b"ACGacg", [0, 1, 2, 0, 1, 2]):
    LUT_BOUNDARY[_ch] = _v


def write_case(directory, name, model_lengths, records, seed=0, consensus=None):
    """-> (fasta path, hmm path).  records: texts; consensus: None (random per model) or one symbol every model repeats.
    Models of an A-only consensus hit all over poly-A text, the terminators and the A padding behind the last record."""
    rng = np.random.default_rng(seed)
    models = []
    for k, L in enumerate(model_lengths):
        cons = np.full(L, consensus, np.uint8) if consensus is not None else rng.integers(0, 4, size=L, dtype=np.uint8)
        models.append(dict(name=f"{name}{k}", acc=f"RF{k:05d}", emissions=synth.emissions_from_consensus(cons, 80 + k + seed),
                           maxl=3 * L + 50, mu=-9.2 + 0.1 * k, lam=0.71))
    fa, hmm = os.path.join(str(directory), name + ".fa"), os.path.join(str(directory), name + ".hmm")
    synth.write_fasta(fa, [(f"seq{j}", t) for j, t in enumerate(records)])
    synth.write_hmm(hmm, models)
    return fa, hmm


def random_text(n, rng):
    return "".join("ACGT"[v] for v in rng.integers(0, 4, size=n))


def raw_hits(fa, hmm, oracle, seed):
    """the packer's layout (srand(seed)), the product's projection, the CPU checker's sweep -> raw records in device order"""
    from havac_amd import havac
    packed, _, _ = havac.pack_fasta(fa, seed=seed)
    table, lens = havac.project_hmm(hmm, 0.02)
    return oracle.ssv(oracle.unpack_2bit(packed), table), lens


def masked_pieces(mask, ncolumns):
    """the column stretches between separator pairs of a pair bitmap (one bit per even column)"""
    bits = np.unpackbits(np.asarray(mask, np.uint8), bitorder="little")[: ncolumns // 2]
    seps = (np.flatnonzero(bits) * 2).tolist()
    pieces, start = [], 0
    for s in seps + [ncolumns]:
        if s > start:
            pieces.append((start, s))
        start = s + 2
    return pieces


def boundary_raw(fa, hmm, p, oracle, both_strands):
    """raw records of a boundary-mode run, from the product's host layout (separator pairs) and its projection with two
    -128 rows behind every model, swept by the checker piece by piece"""
    from havac_amd import havac
    packed, mask, _ = havac.pack_fasta_layout(fa, True, both_strands, seed=1)
    table, lens = havac.project_hmm(hmm, p)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
    sep = np.full((2, 4), -128, np.int8)
    table = np.concatenate([np.concatenate([table[starts[k]:starts[k + 1]], sep]) for k in range(len(lens))])
    sym = oracle.unpack_2bit(packed)
    parts = []
    for a, b in masked_pieces(mask, sym.size):
        r, c = oracle.unpack_hits(oracle.ssv(sym[a:b], table))
        parts.append(oracle.pack_hits(r, c + np.uint64(a)))
    return oracle.device_order(np.concatenate(parts)), lens


def records_of(fa):
    records, cur = [], None
    for line in open(fa):
        if line.startswith(">"):
            if cur is not None:
                records.append("".join(cur))
            cur = []
        else:
            cur.append(line.strip())
    records.append("".join(cur))
    return records
