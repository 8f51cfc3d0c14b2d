"""Havac::searchFastaFile on the GPU: a FASTA file scored in streamed, double-buffered blocks (include/havac_dev.h level 1b)
against one load of the same file (loadSequence + runHardwareClient + getHitsFromFinishedRun) and the CPU checker."""
import ctypes as C

import numpy as np
import pytest

from havac_amd import synth

pytestmark = pytest.mark.gpu

SEG = synth.SEGMENT


def write_inputs(tmp_path, lengths, record_lengths, seed=0, name="in"):
    """models of the given lengths; records with planted homologs, ambiguity codes and lower case"""
    rng = np.random.default_rng(seed)
    models, all_cons = [], []
    for k, L in enumerate(lengths):
        _, cons = synth.dfam_like_model(L, 170 + k + seed)
        all_cons.append(cons)
        models.append(dict(name=f"fam{k}", acc=f"RF{k:05d}", emissions=synth.emissions_from_consensus(cons, 180 + k),
                           maxl=3 * L + 50, mu=-9.2 + 0.1 * k, lam=0.71))
    cons = np.concatenate(all_cons)
    records = []
    for k, n in enumerate(record_lengths):
        s = rng.integers(0, 4, size=n, dtype=np.uint8)
        if n > 400:
            synth.plant_homologs(s, cons, n, every=3000, length=min(cons.size, 300), seed=k)
        text = "".join("ACGT"[v] for v in s)
        if n > 100:
            cut = [int(x) for x in rng.integers(0, n - 10, size=6)]
            for c in cut:
                text = text[:c] + "NRYKMSWBN"[: min(9, n - c)] + text[c + 9:]
            text = text[: n // 2] + text[n // 2:].lower()
        records.append((f"seq{k}", text))
    fa, hmm = tmp_path / f"{name}.fa", tmp_path / f"{name}.hmm"
    synth.write_fasta(str(fa), records)
    synth.write_hmm(str(hmm), models)
    return str(fa), str(hmm)


def one_load(fa, hmm, seed, boundary=False, both=False):
    from havac_amd import havac
    h = havac.Havac(0, 0.02)
    h.setBoundaryMode(boundary)
    h.setBothStrands(both)
    h.loadPhmm(hmm)
    C.CDLL(None).srand(seed)
    h.loadSequence(fa)
    h.runHardwareClient()
    hits, raw = h.getHitsFromFinishedRun(), h.rawHits()
    h.close()
    return hits, raw


def as_tuples(hits):
    return sorted((x.sequenceIndex, x.reverseStrand, x.phmmIndex, x.sequencePosition, x.phmmPosition) for x in hits)


# models of 8000 + 14000 + 18000 rows: the halo of a pass reaches back over more than a block of two or three segments
TALL = [8000, 14000, 18000]
RECORDS = [30000, 9000, 70000, 17, 1, 40000, 300]


@pytest.mark.parametrize("block_segments", [2, 3])
def test_plain_search_equals_one_load_element_for_element(tmp_path, oracle, block_segments):
    from havac_amd import havac
    fa, hmm = write_inputs(tmp_path, TALL, RECORDS, seed=3)
    seed = 97
    want_hits, want_raw = one_load(fa, hmm, seed)
    assert len(want_hits) > 50
    packed, nchars, _ = havac.pack_fasta(fa, seed=seed)
    if block_segments == 2:                                            # (the checker takes ~20 s on the CPU: once)
        table, _ = havac.project_hmm(hmm, 0.02)
        assert np.array_equal(want_raw, oracle.ssv(oracle.unpack_2bit(packed), table))

    h = havac.Havac(0, 0.02)
    h.loadPhmm(hmm)
    C.CDLL(None).srand(seed)
    got = h.searchFastaFile(fa, blockColumns=block_segments * SEG)
    stats = h.lastSearchStats()
    assert np.array_equal(stats["rawHits"], want_raw)                  # global columns, device order, element for element
    assert got == want_hits
    assert stats["columns"] == nchars and stats["records"] == len(RECORDS)
    assert stats["blocks"] == -(-(-(-nchars // SEG) * SEG) // (block_segments * SEG))
    assert stats["recordLengths"].tolist() == RECORDS
    assert stats["readerPeakBytes"] <= (block_segments + 1) * SEG
    # hits lie in many blocks, records are cut by block edges, and the halo is longer than a block
    cols = (want_raw >> np.uint64(14) & np.uint64((1 << 26) - 1)) * np.uint64(SEG) + (want_raw & np.uint64(SEG - 1))
    assert np.unique(cols // np.uint64(block_segments * SEG)).size >= 4
    assert sum(TALL) > block_segments * SEG
    h.close()


def test_search_leaves_the_loaded_sequence_alone(tmp_path):
    from havac_amd import havac
    fa, hmm = write_inputs(tmp_path, [300, 150], [40000, 9000, 20000], seed=5)
    fb, _ = write_inputs(tmp_path, [300, 150], [70000, 500], seed=6, name="other")
    h = havac.Havac(0, 0.02)
    h.loadPhmm(hmm)
    C.CDLL(None).srand(11)
    h.loadSequence(fa)
    h.runHardwareClient()
    before, raw_before = h.getHitsFromFinishedRun(), h.rawHits()
    assert len(before) > 10
    searched = h.searchFastaFile(fb, blockColumns=2 * SEG)
    assert len(searched) > 10
    h.runHardwareClient()
    assert h.getHitsFromFinishedRun() == before and np.array_equal(h.rawHits(), raw_before)
    h.close()


@pytest.mark.parametrize("both", [False, True])
def test_boundary_search_equals_one_load_as_a_multiset(tmp_path, both):
    from havac_amd import havac
    fa, hmm = write_inputs(tmp_path, [300, 1200, 90], [50000, 9000, 130000, 17, 1, 61000, 300], seed=8)
    want, _ = one_load(fa, hmm, 0, boundary=True, both=both)
    assert len(want) > 50 and (both or not any(x.reverseStrand for x in want))
    h = havac.Havac(0, 0.02)
    h.setBoundaryMode(True)
    h.setBothStrands(both)
    h.loadPhmm(hmm)
    got = h.searchFastaFile(fa, blockColumns=20000)                  # records of 50000 and more grow their blocks
    assert as_tuples(got) == as_tuples(want)
    stats = h.lastSearchStats()
    assert stats["records"] == 7 and stats["blocks"] >= 3
    h.close()


def test_on_block_hands_over_every_block_in_file_order(tmp_path):
    from havac_amd import havac
    fa, hmm = write_inputs(tmp_path, TALL, RECORDS, seed=3)
    h = havac.Havac(0, 0.02)
    h.loadPhmm(hmm)
    C.CDLL(None).srand(5)
    whole = h.searchFastaFile(fa, blockColumns=3 * SEG)
    blocks = []
    C.CDLL(None).srand(5)
    assert h.searchFastaFile(fa, blockColumns=3 * SEG, onBlock=blocks.append) == []
    stats = h.lastSearchStats()
    assert len(blocks) == stats["blocks"] and stats["rawHits"].size == 0
    assert [x for b in blocks for x in b] == whole and len(whole) > 50
    ends = np.cumsum(np.array(RECORDS) + 1)
    firsts = [(ends[x.sequenceIndex] - RECORDS[x.sequenceIndex] - 1) + x.sequencePosition for b in blocks for x in b[:1]]
    assert firsts == sorted(firsts)
    h.close()


def test_search_refusals_and_recovery(tmp_path, oracle):
    from havac_amd import havac
    from havac_amd.hw_client import HitOverflowError, LengthError, LogicError
    fa, hmm = write_inputs(tmp_path, [300, 150], [40000, 9000, 20000], seed=5)
    h = havac.Havac(0, 0.02)
    with pytest.raises(LogicError, match="Phmm was not loaded"):
        h.searchFastaFile(fa)
    h.loadPhmm(hmm)
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    with pytest.raises(LengthError):
        h.searchFastaFile(str(empty))
    with pytest.raises(RuntimeError, match="Could not open fasta"):
        h.searchFastaFile(str(tmp_path / "missing.fa"))
    h.setBothStrands(True)
    with pytest.raises(LogicError, match="both strands"):
        h.searchFastaFile(fa)
    h.setBothStrands(False)
    packed, _, _ = havac.pack_fasta(fa, seed=23)
    table, _ = havac.project_hmm(hmm, 0.02)
    want = oracle.ssv(oracle.unpack_2bit(packed), table)
    assert want.size > 10
    C.CDLL(None).srand(23)
    h.loadSequence(fa)
    h.runHardwareClientAsync()
    with pytest.raises(LogicError, match="in flight"):
        h.searchFastaFile(fa)
    h.waitHardwareClientAsync()
    h.getHitsFromFinishedRun()
    assert np.array_equal(h.rawHits(), want)
    # one block overflows the hit capacity: the error names the block, and the handle works afterwards
    h.setHitCapacity(3)
    with pytest.raises(HitOverflowError, match=r"block \d+ of the search"):
        h.searchFastaFile(fa, blockColumns=2 * SEG)
    h.setHitCapacity(1 << 20)
    h.runHardwareClient()
    h.getHitsFromFinishedRun()
    assert np.array_equal(h.rawHits(), want)
    C.CDLL(None).srand(23)
    assert len(h.searchFastaFile(fa, blockColumns=2 * SEG)) > 10
    assert np.array_equal(h.lastSearchStats()["rawHits"], want)
    h.close()
