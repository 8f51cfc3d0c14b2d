"""The checker's resolver (oracle/resolve.py: raw records -> HavacHit fields, restated in numpy) against the product's free
resolver (havac.resolve_hits, host/Havac.cpp) on raw lists the CPU checker finds on files, at the edges a resolver gets
wrong: records of one residue (and hits on the records behind them), a hit on a terminator column, hits in the padding behind the last record, the last row of
the last model, ambiguity codes, no hits at all.  Boundary mode and both strands against expectations worked out record by
record and strand by strand (tests/golden/g8_*, tests/test_gpu_boundary_mode.py).  No GPU."""
import numpy as np
import pytest

from havac_amd import synth
from oracle.cases import LUT_BOUNDARY, boundary_raw, random_text, raw_hits, records_of, write_case
from oracle.resolve import expected_hits, record_layout


def cases(tmp_path):
    rng = np.random.default_rng(3)
    homolog = "A" * 400
    yield "one_residue", write_case(tmp_path, "one_residue", [40, 90, 25], ["A", homolog, "A", "A" * 7, "A", homolog, "C"], 1, 0), 11
    yield "terminators", write_case(tmp_path, "terminators", [30, 12], ["A" * 200, "A" * 7, "A" * 1000], 2, 0), 12
    yield "padding", write_case(tmp_path, "padding", [50], [random_text(500, rng), "A" * 300], 3, 0), 13
    yield "ambiguity", write_case(tmp_path, "ambiguity", [60, 300, 150],
                                  [random_text(2000, rng), "NNNNRYKM" * 30 + "A" * 300 + "NNNN", random_text(700, rng)], 4, 0), 14
    yield "random_models", write_case(tmp_path, "random_models", [70, 300, 33], [random_text(9000, rng), random_text(17, rng)], 5), 15
    yield "no_hits", write_case(tmp_path, "no_hits", [80], ["C" * 50, "G" * 30], 6, 3), 16


def test_the_checker_resolver_equals_the_product_resolver_at_the_edges(tmp_path, oracle):
    from havac_amd import havac
    seen = set()
    for name, (fa, hmm), seed in cases(tmp_path):
        raw, lens = raw_hits(fa, hmm, oracle, seed)
        record_lengths = []
        for line in open(fa):
            if line.startswith(">"):
                record_lengths.append(0)
            else:
                record_lengths[-1] += len(line.strip())
        want = expected_hits(raw, record_lengths, lens)
        got = havac.resolve_hits(fa, hmm, raw)
        assert [(h.sequencePosition, h.sequenceIndex, h.phmmPosition, h.phmmIndex) for h in got] == [w[:4] for w in want], name
        assert not any(w[4] for w in want)
        _, cols = oracle.unpack_hits(raw)
        ends = np.cumsum([n + 1 for n in record_lengths])
        if raw.size == 0:
            seen.add("empty")
        if (cols >= ends[-1]).any():
            seen.add("padding")
            assert len(want) == int((cols < ends[-1]).sum())
        if any(w[0] == record_lengths[w[1]] for w in want):
            seen.add("terminator")
        if any(w[1] > 0 and record_lengths[w[1] - 1] == 1 for w in want):
            seen.add("one_residue")                    # (records of one residue take two columns: the ones behind them count on it)
        if any(w[3] == len(lens) - 1 and w[2] == lens[-1] - 1 for w in want):
            seen.add("last_row_of_last_model")
        if name == "ambiguity" and any(w[1] == 1 for w in want):
            seen.add("ambiguity")
    assert seen == {"empty", "padding", "terminator", "one_residue", "last_row_of_last_model", "ambiguity"}


def test_boundary_mode_resolution_equals_hits_from_ssv_fixtures(tmp_path, oracle):
    """the reference's per-(model, record) SSV on the g8 files (HitsFromSsv, host/test/Ssv.cpp:8-68) is what the checker's
    resolver makes of the raw list of the boundary layout"""
    from conftest import g8_names, load_g8
    names = g8_names()
    assert len(names) >= 6
    for name in names:
        fa, hmm, p, want, _ = load_g8(name, tmp_path)
        raw, lens = boundary_raw(fa, hmm, p, oracle, both_strands=False)
        lengths = [len(t) for t in records_of(fa)]
        got = expected_hits(raw, lengths, lens, boundary=True)
        assert sorted((j, k, pos, row) for pos, j, row, k, _ in got) == want, name
        assert len(got) == len(set(got))


def test_both_strands_resolution_equals_strand_by_strand_expectations(tmp_path, oracle):
    """boundary mode with both strands: every (model, record, strand) triple on its own (test_gpu_boundary_mode.py's
    test_boundary_mode_with_both_strands); the plain layout with both strands: the forward half as the plain resolver sees
    it, the reverse half folded onto the record and mirrored, worked out column by column"""
    from havac_amd import havac
    rng = np.random.default_rng(8)
    fa, hmm = write_case(tmp_path, "strands", [70, 21], [random_text(3000, rng) + "A" * 300, "T" * 200, "C" * 7, "A" * 40], 13, 0)
    table, lens = havac.project_hmm(hmm, 0.02)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
    texts = records_of(fa)
    want = set()
    for j, text in enumerate(texts):
        fwd = LUT_BOUNDARY[np.frombuffer(text.encode(), np.uint8)]
        for strand, residues in ((False, fwd), (True, (3 - fwd)[::-1])):
            sym = np.concatenate([residues, [3]]).astype(np.uint8)           # + terminator column ('T')
            for k in range(len(lens)):
                r, c = oracle.unpack_hits(oracle.ssv(sym, table[starts[k]:starts[k + 1]]))
                for rr, cc in zip(r.tolist(), c.tolist()):
                    pos = len(text) - 1 - cc if (strand and cc < len(text)) else cc
                    want.add((pos, j, rr, k, strand))
    raw, _ = boundary_raw(fa, hmm, 0.02, oracle, both_strands=True)
    got = expected_hits(raw, [len(t) for t in texts], lens, boundary=True, both_strands=True)
    assert len(got) == len(set(got)) and len(want) > 40 and any(w[4] for w in want)
    assert set(got) == want
    # the plain layout, both strands: the forward half is the plain layout of the file, resolved by the product's free
    # resolver; the reverse half is the plain layout of the reverse-complemented records (same lengths: the same columns),
    # resolved the same way on a file of those records, where a position counts from the record's far end
    packed, _, nf = havac.pack_fasta_layout(fa, False, True, seed=2)
    lengths = [len(t) for t in texts]
    assert nf == record_layout(lengths)[1]
    sym = oracle.unpack_2bit(packed)
    raw = oracle.ssv(sym, table)
    rows, cols = oracle.unpack_hits(raw)
    reverse = cols >= np.uint64(nf)
    rc_fa = str(tmp_path / "strands_rc.fa")
    synth.write_fasta(rc_fa, [(f"rc{j}", t[::-1].translate(str.maketrans("ACGT", "TGCA"))) for j, t in enumerate(texts)])
    want_f = [(h.sequencePosition, h.sequenceIndex, h.phmmPosition, h.phmmIndex, False) for h in havac.resolve_hits(fa, hmm, raw[~reverse])]
    rc_raw = oracle.pack_hits(rows[reverse], cols[reverse] - np.uint64(nf))
    want_r = []
    for h in havac.resolve_hits(rc_fa, hmm, rc_raw):
        n = lengths[h.sequenceIndex]
        want_r.append((n - 1 - h.sequencePosition if h.sequencePosition < n else n, h.sequenceIndex, h.phmmPosition, h.phmmIndex, True))
    got = expected_hits(raw, lengths, lens, both_strands=True)
    assert [g for g in got if not g[4]] == want_f and [g for g in got if g[4]] == want_r
    assert want_f and want_r
    # and a reverse hit names the residue its cell read: the complement of the file's residue at sequencePosition
    reverse_columns = cols[reverse].astype(np.int64)
    resolved = iter(g for g in got if g[4])
    starts_rc = record_layout(lengths)[0]
    for c in reverse_columns.tolist():
        j = int(np.searchsorted(starts_rc + np.array(lengths) + 1, c - nf, side="right"))
        if j == len(lengths):
            continue                                          # padding behind the last record
        pos, jj = next(resolved)[:2]
        assert jj == j
        if pos < lengths[j]:
            assert sym[c] == 3 - LUT_BOUNDARY[ord(texts[j][pos])]


@pytest.mark.parametrize("boundary", [False, True])
def test_an_empty_list_resolves_to_nothing(boundary):
    assert expected_hits(np.zeros(0, np.uint64), [5, 1], [10, 3], boundary=boundary, both_strands=True) == []
