"""The streamed search's host layers without a GPU: the block reader (havac_amd/csrc/host/FastaStream.h) against FastaVector's
whole-file read, its per-block patches against the whole file's, and the block planner (include/havac_dev.h: havac_stream_block)
against the shard windows it must reproduce."""
import ctypes as C

import numpy as np
import pytest

from havac_amd import _lib, havac

SEG = 12288


def write_awkward_fasta(path, seed=0):
    """ragged and empty records, long and short lines, CRLF and blank lines, lower case, every ambiguity code, residues before
    the first header"""
    rng = np.random.default_rng(seed)
    ambiguity = "NRYSWKMBDHVnryswkmbdhvXx-"
    parts = ["acgtNNRY\n", "\n"]
    for k, n in enumerate([0, 1, 37, 5000, 0, 130, 25000, 2, 9999, 0, 61, 3]):
        seq = "".join(rng.choice(list("ACGTacgt"), size=n)) if n else ""
        if n > 10:
            pos = rng.integers(0, n, size=min(12, n // 3))
            seq = list(seq)
            for p in pos:
                seq[p] = ambiguity[int(rng.integers(0, len(ambiguity)))]
            seq = "".join(seq)
        width = [60, 1, 7, 80, 1000, 13][k % 6]
        eol = "\r\n" if k % 4 == 3 else "\n"
        parts.append(f">rec{k} description {k}{eol}")
        for i in range(0, len(seq), width):
            line = seq[i:i + width]
            if k % 5 == 2 and len(line) > 4:
                line = line[:2] + " \t" + line[2:]          # blanks inside a line are dropped
            parts.append(line + eol)
        if k % 3 == 1:
            parts.append(eol)
    with open(path, "w", newline="") as f:
        f.write("".join(parts))
    return str(path)


def whole_file(path, seed):
    chars, cols, syms = havac.text_and_patches(path, seed=seed)
    ends = np.flatnonzero(chars == 0).astype(np.uint64) + 1
    return chars, ends, cols, syms


@pytest.mark.parametrize("block", [1, 2, 7, 4096, SEG, 3 * SEG + 5, 1 << 30])
def test_reader_blocks_concatenate_to_the_whole_file(tmp_path, block):
    fa = write_awkward_fasta(tmp_path / "a.fa", seed=block % 97)
    chars, ends, _, _ = whole_file(fa, seed=1)
    got = havac.read_fasta_blocks(fa, block, seed=1)
    assert got["chars"] == chars.tobytes()
    assert np.array_equal(got["record_ends"], ends)
    sizes = np.diff(np.concatenate([[0], got["block_ends"]]))
    assert sizes.size and (sizes[:-1] == block).all() and 0 < sizes[-1] <= block    # every block full but the last
    # the reader holds one block at a time: well inside two blocks plus a look-ahead segment plus a line
    assert got["peak"] <= min(block, chars.size)


@pytest.mark.parametrize("block", [1, 100, 6000, SEG, 1 << 30])
def test_reader_record_blocks_hold_whole_records(tmp_path, block):
    fa = write_awkward_fasta(tmp_path / "a.fa", seed=3)
    chars, ends, _, _ = whole_file(fa, seed=2)
    got = havac.read_fasta_blocks(fa, block, whole_records=True, seed=2)
    assert got["chars"] == chars.tobytes()
    assert np.array_equal(got["record_ends"], ends)
    assert set(got["block_ends"].tolist()) <= set(ends.tolist())        # blocks end at record ends
    starts = np.concatenate([[0], got["block_ends"][:-1]])
    sizes = got["block_ends"] - starts
    assert (sizes[:-1] >= block).all()
    # a block grows only by the record it stopped in: without that record's last piece it would have been too short
    for s, e in zip(starts[:-1], got["block_ends"][:-1]):
        inside = ends[(ends > s) & (ends < e)]
        assert inside.size == 0 or inside.max() - s < block
    longest = int(np.diff(np.concatenate([[0], ends])).max())
    assert got["peak"] <= max(block, 0) + longest


@pytest.mark.parametrize("seed", [0, 7, 12345])
@pytest.mark.parametrize("block", [1, 5, SEG, 1 << 30])
def test_per_block_patches_equal_the_whole_files(tmp_path, seed, block):
    fa = write_awkward_fasta(tmp_path / "a.fa", seed=seed)
    _, _, cols, syms = whole_file(fa, seed=seed)
    assert cols.size > 50
    got = havac.read_fasta_blocks(fa, block, seed=seed)
    assert np.array_equal(got["patch_columns"], cols)
    assert np.array_equal(got["patch_symbols"], syms)


def test_reader_of_an_empty_file_reads_nothing(tmp_path):
    fa = tmp_path / "empty.fa"
    fa.write_text("")
    got = havac.read_fasta_blocks(str(fa), SEG)
    assert got["chars"] == b"" and got["record_ends"].size == 0 and got["block_ends"].size == 0
    with pytest.raises(RuntimeError):
        havac.read_fasta_blocks(str(tmp_path / "missing.fa"), SEG)


def plan(block_columns, nrows, k, nsymbols):
    L = _lib.load()
    v = [C.c_uint64(0) for _ in range(4)]
    rc = L.havac_stream_block(block_columns, nrows, k, nsymbols, *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def shard_window(nsymbols, nrows, shard, nshards):
    L = _lib.load()
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert L.havac_ssv_shard_window(nsymbols, nrows, shard, nshards, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("nrows", [1, 40, 5000, 100_000, 1_000_000])
@pytest.mark.parametrize("block_segments", [1, 2, 3, 16])
def test_planner_tiles_the_database_and_covers_what_each_pass_reads(nrows, block_segments):
    B = block_segments * SEG
    for nseg in (1, block_segments, 5 * block_segments, 5 * block_segments + 1, 37):
        N = nseg * SEG
        at, k = 0, 0
        while at < N:
            rc, (ob, oe, first, end) = plan(B, nrows, k, N)
            assert rc == 0
            assert ob == at and oe == min(N, at + B) and ob % SEG == 0 and oe % SEG == 0
            assert first % SEG == 0 and end % SEG == 0 and first <= ob and oe <= end <= N
            # the halo of the diagonals that reach the block, nrows - 1 columns, and more for the tiling
            assert first <= max(0, ob - (nrows - 1))
            # exactly the window of the same columns as a shard, where blocks and shards coincide
            if N % B == 0:
                assert (first, end) == shard_window(N, nrows, k, N // B)
            # while the end is not known, the same halo and the look-ahead of a database that goes on
            rc, (ob2, oe2, first2, end2) = plan(B, nrows, k, 0)
            assert rc == 0 and (ob2, oe2, first2) == (ob, ob + B, first) and end2 == ob + B + SEG
            if oe < N:
                assert end == min(N, end2)
            at, k = oe, k + 1
        assert plan(B, nrows, k, N)[0] == _lib.E_ARGUMENT             # no block past the end


def test_planner_halo_spans_several_blocks():
    B, nrows = 2 * SEG, 100_000
    rc, (ob, oe, first, end) = plan(B, nrows, 20, 0)
    assert rc == 0 and ob - first >= nrows - 1 and (ob - first) // B >= 4


def test_planner_refuses_past_the_segment_field():
    assert plan(SEG, 100, (1 << 26) - 1, 0)[0] == 0
    assert plan(SEG, 100, 1 << 26, 0)[0] == _lib.E_LENGTH
    assert plan(SEG, 100, 0, (1 << 26) * SEG)[0] == 0
    assert plan(SEG, 100, 0, ((1 << 26) + 1) * SEG)[0] == _lib.E_LENGTH
    assert plan(4 * SEG, 100, (1 << 24), 0)[0] == _lib.E_LENGTH
    for bad in ((0, 100, 0, 0), (SEG + 1, 100, 0, 0), (SEG, 0, 0, 0), (SEG, 100, 0, 100)):
        assert plan(*bad)[0] == _lib.E_ARGUMENT
