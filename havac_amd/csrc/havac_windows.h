// havac_windows.h -- a finished run's hit windows made on the GPU (havac_dev_compute_windows; Havac::getDeviceWindowsFromFinishedRun).
//
// Internal to havac_dev.hip and havac_windows.hip (not ABI: include/havac_dev.h holds that).  The records of one GPU's list are
// taken in chunks of at most `chunk` records; every chunk is resolved, sorted and merged on the GPU into windows sorted by
// (record, strand, model, start), and only those windows are copied to the host.  join_window_lists merges sorted lists --
// the chunks of one GPU, the GPUs of one handle -- again as weighted intervals, which gives what one merge over all hits gives.
#pragma once

#include <algorithm>
#include <cstdint>
#include <deque>
#include <string>
#include <vector>

#include "hip_memory.h"

namespace havac {

// One window (or one hit's stretch before the merge).  key = record << 25 | reverse << 24 | model: key order is the output order
// record, strand (forward first), model.
struct WindowItem {
    uint64_t key, start, end;            // start, end: inclusive positions on the record
    uint32_t phmm_first, phmm_last, hit_count, pad;
};
constexpr unsigned kWindowModelBits = 24, kWindowStrandBit = 24, kWindowRecordShift = 25;
inline uint64_t window_key(uint64_t record, bool reverse, uint64_t model) {
    return record << kWindowRecordShift | (uint64_t)reverse << kWindowStrandBit | model;
}

// What a run's records are resolved against (the tables of havac_dev_compute_windows), as host arrays.
struct WindowTables {
    const uint64_t* record_ends = nullptr;      // FASTA end position (one past the terminator) of every record
    uint32_t nrecords = 0;
    const uint32_t* model_lengths = nullptr;
    uint32_t nmodels = 0;
    const uint64_t* record_starts = nullptr;    // boundary mode: first column of every record ...
    const uint64_t* record_columns = nullptr;   // ... and its columns (residues + terminator); NULL: the plain layout
    const uint32_t* model_starts = nullptr;     // boundary mode: first row of every model
    uint64_t forward_columns = 0;               // both strands: columns of the forward half; 0: one strand
    uint32_t flank = 0;
};

constexpr uint64_t kDefaultWindowChunk = 1ull << 24;     // records per chunk: C2's list (1.0e6) is one chunk
constexpr uint64_t kMaxWindowChunk = 1ull << 31;         // (32-bit indices inside a chunk)

// The device memory of one GPU's window merges (owned by its DevicePart): the resolve tables of the last call and the per-chunk
// scratch, grown to the largest chunk seen and kept.
struct WindowScratch {
    DeviceBuffer<uint64_t> d_ends, d_lengths, d_starts, d_columns;      // per record (d_lengths: residues)
    DeviceBuffer<uint32_t> d_prefix, d_model_lengths, d_model_starts;   // per model (d_prefix: nmodels + 1 prefix sums)
    DeviceBuffer<WindowItem> items, sorted;                             // chunk x 40 B each
    DeviceBuffer<uint64_t> keys;                                        // 2 x chunk: the start keys, then the group keys
    DeviceBuffer<uint64_t> pairs;                                       // 2 x chunk: (key, end) pairs before and after the scan
    DeviceBuffer<uint32_t> index;                                       // 2 x chunk: permutation, then heads and window numbers
    DeviceBuffer<uint8_t> tmp;                                          // rocPRIM's temporary storage
    DeviceBuffer<uint64_t> count;                                       // windows of the chunk (1 word)
    uint64_t capacity = 0;                                              // records a chunk may hold with the buffers above
    uint64_t high_water = 0;                                            // largest number of bytes the buffers above held at once
    uint64_t read_back = 0;                                             // bytes of windows copied to the host (the caller resets it)
    // of the last upload_window_tables
    uint32_t nrecords = 0, nmodels = 0;
    bool boundary = false;
    uint64_t forward_columns = 0;
    uint32_t flank = 0;
    unsigned start_bits = 1, key_bits = kWindowRecordShift + 1;

    uint64_t bytes() const;
};

// Copies the tables to the current device (on `stream`, complete on return).
int upload_window_tables(std::string& err, WindowScratch& s, const WindowTables& t, hipStream_t stream);
// The windows of `n` records in device memory (a list in device order; any order will do), appended to `lists` as sorted lists
// of at most `chunk` records' windows each.  On the current device, on `stream`; complete on return.
int windows_of_records(std::string& err, WindowScratch& s, const uint64_t* d_records, uint64_t n, uint64_t chunk, hipStream_t stream,
                       std::vector<std::vector<WindowItem>>& lists);
// A window list on the host, in blocks: a reader copies it out in order and each block is freed once it has been copied, so the
// list and the caller's copy of it are never both whole in host memory (havac_dev_read_windows).
struct WindowBlocks {
    std::deque<std::vector<WindowItem>> blocks;
    uint64_t total = 0;                  // windows in all
    uint64_t served = 0;                 // windows copied out so far
    size_t front_served = 0;             // of them, in blocks.front()
    // copies the next min(n, total - served) windows to `put(i, window)` (i from 0) and frees the blocks passed; -> how many
    template <typename Put>
    uint64_t take(uint64_t n, Put&& put) {
        uint64_t done = 0;
        while (done < n && !blocks.empty()) {
            const std::vector<WindowItem>& b = blocks.front();
            const size_t k = (size_t)std::min<uint64_t>(n - done, b.size() - front_served);
            for (size_t i = 0; i < k; i++) put(done + i, b[front_served + i]);
            done += k; front_served += k;
            if (front_served == b.size()) { blocks.pop_front(); front_served = 0; }
        }
        served += done;
        return done;
    }
};

// Lists each sorted by (key, start), each merged -> one merged list in the same order.  `lists` is consumed: every input list is
// freed as soon as the merge has passed its end, so the host holds at most the inputs not yet passed plus the output.
WindowBlocks join_window_lists(std::vector<std::vector<WindowItem>>& lists);

}  // namespace havac
