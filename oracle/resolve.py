"""The hit resolver restated in numpy: raw 64-bit records -> the fields of the HavacHit list `Havac::getHitsFromFinishedRun`
returns (host/Havac.cpp:104-187 and the additions of this project's `Havac::fetchHits`), worked out from the layouts and not
by the product's code.  Test infrastructure: the product never imports it (tests/test_boundary.py keeps it that way)."""
from __future__ import annotations

import numpy as np

SEGMENT = 12 * 1024
SEPARATOR_COLUMNS = 2          # boundary mode: a separator pair behind every record (on an even column)
SEPARATOR_ROWS = 2             # boundary mode: two rows of -128 behind every model


def _columns_and_rows(raw):
    raw = np.asarray(raw, dtype=np.uint64)
    inseg = (raw & np.uint64(0x3FFF)).astype(np.int64)
    seg = ((raw >> np.uint64(14)) & np.uint64(0x3FFFFFF)).astype(np.int64)
    return seg * SEGMENT + inseg, (raw >> np.uint64(40)).astype(np.int64)


def record_layout(record_lengths, boundary=False):
    """-> (first column of every record, columns the forward strand takes: whole segments).  A record takes its residues and
    one terminator column; in boundary mode it is followed by padding to an even column and a separator pair."""
    starts, at = [], 0
    for n in record_lengths:
        starts.append(at)
        at += int(n) + 1
        if boundary:
            at += at & 1
            at += SEPARATOR_COLUMNS
    return np.array(starts, np.int64), -(-at // SEGMENT) * SEGMENT


def model_layout(model_lengths, boundary=False):
    """-> first row of every model (boundary mode: two separator rows behind every model)"""
    gap = SEPARATOR_ROWS if boundary else 0
    lengths = np.asarray(model_lengths, np.int64)
    return np.concatenate([[0], np.cumsum(lengths + gap)[:-1]]).astype(np.int64) if lengths.size else np.zeros(0, np.int64)


def expected_hits(raw, record_lengths, model_lengths, *, boundary=False, both_strands=False, record_starts=None,
                  model_starts=None, forward_columns=None):
    """raw records in device order -> [(sequencePosition, sequenceIndex, phmmPosition, phmmIndex, reverseStrand)] in the same
    order.  record_lengths: residues per record (without the terminator); model_lengths: rows per model.  Dropped: columns at or
    past the end of the last record (padding), and in boundary mode separator and padding columns and separator rows.  A hit
    on a record's terminator column resolves to position == the record's length.  Both strands: columns from
    `forward_columns` on (default: the forward layout rounded up to whole segments) are the reverse complement of the forward
    layout; such a hit is folded onto the forward column and its position mirrored (n - 1 - position; the terminator stays)."""
    record_lengths = np.asarray(record_lengths, np.int64)
    if record_lengths.size == 0:
        raise ValueError("a run has at least one record")
    model_lengths = np.asarray(model_lengths, np.int64)
    layout_starts, nf = record_layout(record_lengths, boundary)
    if record_starts is None:
        record_starts = layout_starts
    record_starts = np.asarray(record_starts, np.int64)
    if model_starts is None:
        model_starts = model_layout(model_lengths, boundary)
    model_starts = np.asarray(model_starts, np.int64)
    if forward_columns is None:
        forward_columns = nf
    cols, rows = _columns_and_rows(raw)
    reverse = (cols >= forward_columns) if both_strands else np.zeros(cols.size, bool)
    cols = np.where(reverse, cols - forward_columns, cols)
    if boundary:
        j = np.searchsorted(record_starts, cols, side="right") - 1
        k = np.searchsorted(model_starts, rows, side="right") - 1
        keep = (j >= 0) & (k >= 0)
        j, k = np.maximum(j, 0), np.maximum(k, 0)
        pos, mpos = cols - record_starts[j], rows - model_starts[k]
        keep &= (pos <= record_lengths[j]) & (mpos < model_lengths[k])    # not a separator / padding column, not a separator row
    else:
        ends = record_starts + record_lengths + 1
        j = np.searchsorted(ends, cols, side="right")
        keep = j < ends.size                                               # not the padding behind the last record
        j = np.minimum(j, ends.size - 1)
        pos = cols - record_starts[j]
        prefix = np.concatenate([[0], np.cumsum(model_lengths)])
        k = np.searchsorted(prefix, rows, side="right") - 1
        mpos = rows - prefix[k]
    pos = np.where(reverse & (pos < record_lengths[j]), record_lengths[j] - 1 - pos, pos)
    return [(int(a), int(b), int(c), int(d), bool(e))
            for a, b, c, d, e in zip(pos[keep], j[keep], mpos[keep], k[keep], reverse[keep])]
