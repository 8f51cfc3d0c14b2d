// havac_windows.hip -- a finished run's hit windows made on the GPU (see havac_windows.h; the host path they must equal element for
// element is havacMergeHitsToWindows over Havac::fetchHits, host/Havac.cpp).
//
// One chunk of records, all on the GPU, one stream:
//   1. resolve_records: record -> (group key, start, end, model position) -- the resolver of fetchHits (plain or boundary layout,
//      both strands folded and mirrored) and the stretch of havacMergeHitsToWindows.  A record that resolves to nothing gets the
//      key `nrecords << 25`, above every real key: it sorts behind them and its window is dropped on the host.
//   2. two stable radix sorts of a permutation: by start, then by group key -> (key, start) order.
//   3. a segmented max-scan of the ends within each key: a record starts a new window where the key changes or where its start
//      lies more than one past every end before it (windows that only touch join, as on the host).
//   4. a sum scan of those heads numbers the windows; reduce_by_key over the numbers joins each window's records (max end, min /
//      max model position, summed count).
// Only the windows are copied to the host.  Plain C++ stores only: no scalar-memory store or scalar atomic is needed anywhere.
#include <algorithm>
#include <cstring>
#include <queue>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "havac_windows.h"

namespace havac {
namespace {

constexpr unsigned kThreads = 256;

unsigned bit_width(uint64_t v) {
    unsigned b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>((n + kThreads - 1) / kThreads, 1u << 16); }

// first index in [0, n) whose entry is greater than v (std::upper_bound)
template <typename T>
__device__ uint64_t upper_bound(const T* a, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct ResolveArgs {
    const uint64_t* ends;            // plain layout: record_ends
    const uint64_t* lengths;         // residues of every record (the window's clip and the reverse strand's mirror)
    const uint64_t* starts;          // boundary layout: first column of every record ...
    const uint64_t* columns;         // ... and its columns (residues + terminator)
    const uint32_t* prefix;          // plain layout: nmodels + 1 prefix sums of the model lengths
    const uint32_t* model_lengths;
    const uint32_t* model_starts;    // boundary layout
    uint32_t nrecords, nmodels;
    uint64_t forward_columns;        // 0: one strand
    uint32_t flank;
    int boundary;
};

__global__ void resolve_records(const uint64_t* __restrict__ records, uint64_t n, ResolveArgs a, WindowItem* __restrict__ items,
                                uint64_t* __restrict__ start_keys, uint64_t* __restrict__ group_keys, uint32_t* __restrict__ index) {
    const uint64_t dropped = (uint64_t)a.nrecords << kWindowRecordShift;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t rec = records[i];
        uint64_t column = ((rec >> 14) & 0x3ffffffull) * (uint64_t)HAVAC_SEGMENT_COLUMNS + (rec & 0x3fffull);
        const uint64_t row = rec >> 40;
        bool reverse = false;
        if (a.forward_columns && column >= a.forward_columns) { column -= a.forward_columns; reverse = true; }
        bool keep = true;
        uint64_t j = 0, k = 0, position = 0, model_position = 0;
        if (!a.boundary) {
            j = upper_bound(a.ends, a.nrecords, column);                          // the first record whose end lies beyond the column
            if (j == a.nrecords) keep = false;                                    // the padding after the last record
            else position = column - (j ? a.ends[j - 1] : 0);
            k = upper_bound(a.prefix, (uint64_t)a.nmodels + 1, row) - 1;          // largest prefix sum <= the row (prefix[0] = 0)
            model_position = row - a.prefix[k];
            if (k >= a.nmodels) keep = false;                                     // rows past the last model
        } else {
            j = upper_bound(a.starts, a.nrecords, column);
            k = upper_bound(a.model_starts, a.nmodels, row);
            if (j == 0 || k == 0) keep = false;
            else {
                j--; k--;
                position = column - a.starts[j];
                model_position = row - a.model_starts[k];
                if (position >= a.columns[j] || model_position >= a.model_lengths[k]) keep = false;   // separator / padding column or row
            }
        }
        WindowItem w{dropped, 0, 0, 0, 0, 0, 0};
        if (keep) {
            const uint64_t len = a.lengths[j], L = a.model_lengths[k];
            if (reverse && position < len) position = len - 1 - position;      // the terminator column stays
            if (len == 0 || L == 0) keep = false;
            else {
                const uint64_t p = position < len - 1 ? position : len - 1;    // a hit on the terminator column
                const uint64_t q = model_position < L - 1 ? model_position : L - 1;
                const uint64_t before = (reverse ? L - 1 - q : q) + a.flank;
                const uint64_t after = (reverse ? q : L - 1 - q) + a.flank;
                w.key = j << kWindowRecordShift | (uint64_t)reverse << kWindowStrandBit | k;
                w.start = p > before ? p - before : 0;
                w.end = p + after < len - 1 ? p + after : len - 1;
                w.phmm_first = w.phmm_last = (uint32_t)q;
                w.hit_count = 1;
            }
        }
        items[i] = w;
        start_keys[i] = w.start;
        group_keys[i] = w.key;
        index[i] = (uint32_t)i;
    }
}

__global__ void gather_keys(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ index, uint64_t* __restrict__ out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = keys[index[i]];
}

struct KeyEnd { uint64_t key, end; };

__global__ void gather_items(const WindowItem* __restrict__ items, const uint32_t* __restrict__ index, WindowItem* __restrict__ sorted,
                             KeyEnd* __restrict__ pairs, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const WindowItem w = items[index[i]];
        sorted[i] = w;
        pairs[i] = KeyEnd{w.key, w.end};
    }
}

// 1 where a window begins: the first record of its key, or one that starts more than one past every end before it in its key
__global__ void window_heads(const WindowItem* __restrict__ sorted, const KeyEnd* __restrict__ running, uint32_t* __restrict__ head, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        head[i] = i == 0 || running[i - 1].key != sorted[i].key || sorted[i].start > running[i - 1].end + 1;
}

// (sorted by key) the largest end so far within the key
struct SegmentedMax {
    __host__ __device__ KeyEnd operator()(const KeyEnd& a, const KeyEnd& b) const {
        return KeyEnd{b.key, a.key == b.key && a.end > b.end ? a.end : b.end};
    }
};

// two stretches of one window -> one (every field commutative: the order reduce_by_key combines them in does not matter)
struct JoinWindows {
    __host__ __device__ WindowItem operator()(const WindowItem& a, const WindowItem& b) const {
        WindowItem w = a;
        w.start = a.start < b.start ? a.start : b.start;
        w.end = a.end > b.end ? a.end : b.end;
        w.phmm_first = a.phmm_first < b.phmm_first ? a.phmm_first : b.phmm_first;
        w.phmm_last = a.phmm_last > b.phmm_last ? a.phmm_last : b.phmm_last;
        w.hit_count = a.hit_count + b.hit_count;                 // (32 bits, as HavacWindow::hitCount)
        return w;
    }
};

// rocPRIM's two-call protocol with the scratch's temporary buffer grown as needed
template <typename Call>
int with_tmp(std::string& err, WindowScratch& s, hipStream_t stream, const char* what, Call&& call) {
    size_t need = 0;
    if (hipError_t e = call((void*)nullptr, need); e != hipSuccess) { err = hip_msg(what, e); return HAVAC_E_RUNTIME; }
    if (s.tmp.capacity() < need) {
        HIP_TRY(err, s.tmp.grow(need + need / 4, stream));
        s.high_water = std::max(s.high_water, s.bytes());
    }
    size_t bytes = s.tmp.capacity();
    if (hipError_t e = call((void*)s.tmp.get(), bytes); e != hipSuccess) { err = hip_msg(what, e); return HAVAC_E_RUNTIME; }
    return HAVAC_OK;
}

int ensure_capacity(std::string& err, WindowScratch& s, uint64_t n, hipStream_t stream) {
    if (s.capacity >= n) return HAVAC_OK;
    s.capacity = 0;                                  // (the buffer that gates the group first: a failed grow regrows them all)
    HIP_TRY(err, s.items.grow(n, stream));
    HIP_TRY(err, s.sorted.grow(n));
    HIP_TRY(err, s.keys.grow(2 * n));
    HIP_TRY(err, s.pairs.grow(2 * n));
    HIP_TRY(err, s.index.grow(2 * n));
    if (s.count.capacity() == 0) HIP_TRY(err, s.count.grow(1));
    s.capacity = n;
    s.high_water = std::max(s.high_water, s.bytes());
    return HAVAC_OK;
}

int merge_chunk(std::string& err, WindowScratch& s, const ResolveArgs& args, const uint64_t* d_records, uint64_t n, hipStream_t stream,
                std::vector<WindowItem>& out) {
    if (int rc = ensure_capacity(err, s, n, stream)) return rc;
    const unsigned grid = grid_for(n);
    uint64_t* const start_in = s.keys.get();
    uint64_t* const start_out = s.keys.get() + n;
    uint64_t* const key_in = s.keys.get() + n;               // (the start keys are done with by then)
    uint64_t* const key_out = s.keys.get();
    uint32_t* const perm_a = s.index.get();
    uint32_t* const perm_b = s.index.get() + n;
    uint64_t* const group_keys = reinterpret_cast<uint64_t*>(s.pairs.get());     // until the gather; then the pairs
    KeyEnd* const pairs_in = reinterpret_cast<KeyEnd*>(s.pairs.get());
    KeyEnd* const pairs_out = reinterpret_cast<KeyEnd*>(s.keys.get());
    hipLaunchKernelGGL(resolve_records, dim3(grid), dim3(kThreads), 0, stream, d_records, n, args, s.items.get(), start_in, group_keys, perm_a);
    if (int rc = with_tmp(err, s, stream, "sorting by start", [&](void* t, size_t& b) {
            return rocprim::radix_sort_pairs(t, b, start_in, start_out, perm_a, perm_b, (size_t)n, 0, s.start_bits, stream);
        })) return rc;
    hipLaunchKernelGGL(gather_keys, dim3(grid), dim3(kThreads), 0, stream, group_keys, perm_b, key_in, n);
    if (int rc = with_tmp(err, s, stream, "sorting by record, strand and model", [&](void* t, size_t& b) {
            return rocprim::radix_sort_pairs(t, b, key_in, key_out, perm_b, perm_a, (size_t)n, 0, s.key_bits, stream);
        })) return rc;
    hipLaunchKernelGGL(gather_items, dim3(grid), dim3(kThreads), 0, stream, s.items.get(), perm_a, s.sorted.get(), pairs_in, n);
    if (int rc = with_tmp(err, s, stream, "the running end", [&](void* t, size_t& b) {
            return rocprim::inclusive_scan(t, b, pairs_in, pairs_out, (size_t)n, SegmentedMax(), stream);
        })) return rc;
    uint32_t* const heads = perm_a;
    uint32_t* const numbers = perm_b;
    hipLaunchKernelGGL(window_heads, dim3(grid), dim3(kThreads), 0, stream, s.sorted.get(), pairs_out, heads, n);
    if (int rc = with_tmp(err, s, stream, "numbering the windows", [&](void* t, size_t& b) {
            return rocprim::inclusive_scan(t, b, heads, numbers, (size_t)n, rocprim::plus<uint32_t>(), stream);
        })) return rc;
    if (int rc = with_tmp(err, s, stream, "joining the windows", [&](void* t, size_t& b) {
            return rocprim::reduce_by_key(t, b, numbers, s.sorted.get(), (size_t)n, heads, s.items.get(), s.count.get(), JoinWindows(),
                                          rocprim::equal_to<uint32_t>(), stream);
        })) return rc;
    HIP_TRY(err, hipGetLastError());
    uint64_t windows = 0;
    HIP_TRY(err, hipMemcpyAsync(&windows, s.count.get(), sizeof windows, hipMemcpyDeviceToHost, stream));
    HIP_TRY(err, hipStreamSynchronize(stream));
    if (windows > n) { err = "window merge: more windows than records"; return HAVAC_E_RUNTIME; }
    out.resize(windows);
    if (windows) {
        HIP_TRY(err, hipMemcpyAsync(out.data(), s.items.get(), windows * sizeof(WindowItem), hipMemcpyDeviceToHost, stream));
        HIP_TRY(err, hipStreamSynchronize(stream));
        s.read_back += windows * sizeof(WindowItem);
    }
    // the records that resolved to nothing: one window behind all others, with the key no record has
    if (!out.empty() && out.back().key == (uint64_t)s.nrecords << kWindowRecordShift) out.pop_back();
    return HAVAC_OK;
}

}  // namespace

uint64_t WindowScratch::bytes() const {
    return (items.capacity() + sorted.capacity()) * sizeof(WindowItem) + (keys.capacity() + pairs.capacity() + count.capacity()) * 8 +
           index.capacity() * 4 + tmp.capacity() +
           (d_ends.capacity() + d_lengths.capacity() + d_starts.capacity() + d_columns.capacity()) * 8 +
           (d_prefix.capacity() + d_model_lengths.capacity() + d_model_starts.capacity()) * 4;
}

namespace {
// `n` host values into `buf`, which only grows (a free would wait for the whole device: the next run may be in flight)
template <typename T>
hipError_t put_table(DeviceBuffer<T>& buf, const T* src, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (buf.capacity() < n) {
        if (hipError_t e = buf.grow(n + n / 4, stream); e != hipSuccess) return e;
    }
    return hipMemcpyAsync(buf.get(), src, n * sizeof(T), hipMemcpyHostToDevice, stream);
}
}  // namespace

int upload_window_tables(std::string& err, WindowScratch& s, const WindowTables& t, hipStream_t stream) {
    const uint32_t R = t.nrecords, M = t.nmodels;
    std::vector<uint64_t> lengths(R);
    uint64_t longest = 0;
    for (uint32_t j = 0; j < R; j++) {                      // residues: the end is one past the terminator
        const uint64_t begin = j ? t.record_ends[j - 1] : 0;
        lengths[j] = t.record_ends[j] > begin ? t.record_ends[j] - begin - 1 : 0;
        longest = std::max(longest, lengths[j]);
    }
    std::vector<uint32_t> prefix(M + 1, 0);
    for (uint32_t k = 0; k < M; k++) prefix[k + 1] = prefix[k] + t.model_lengths[k];
    s.boundary = t.record_starts != nullptr;
    HIP_TRY(err, put_table(s.d_ends, t.record_ends, R, stream));
    HIP_TRY(err, put_table(s.d_lengths, lengths.data(), R, stream));
    HIP_TRY(err, put_table(s.d_starts, t.record_starts, s.boundary ? R : 0, stream));
    HIP_TRY(err, put_table(s.d_columns, t.record_columns, s.boundary ? R : 0, stream));
    HIP_TRY(err, put_table(s.d_prefix, prefix.data(), M + 1, stream));
    HIP_TRY(err, put_table(s.d_model_lengths, t.model_lengths, M, stream));
    HIP_TRY(err, put_table(s.d_model_starts, t.model_starts, s.boundary ? M : 0, stream));
    HIP_TRY(err, hipStreamSynchronize(stream));             // (copies from pageable memory the caller may free on return)
    s.high_water = std::max(s.high_water, s.bytes());
    s.nrecords = R; s.nmodels = M;
    s.forward_columns = t.forward_columns;
    s.flank = t.flank;
    s.start_bits = std::max(1u, bit_width(longest));        // starts < the longest record
    s.key_bits = kWindowRecordShift + std::max(1u, bit_width(R));    // keys <= nrecords << 25 (the dropped records' key)
    return HAVAC_OK;
}

int windows_of_records(std::string& err, WindowScratch& s, const uint64_t* d_records, uint64_t n, uint64_t chunk, hipStream_t stream,
                       std::vector<std::vector<WindowItem>>& lists) {
    ResolveArgs args{s.d_ends.get(), s.d_lengths.get(), s.d_starts.get(), s.d_columns.get(), s.d_prefix.get(), s.d_model_lengths.get(),
                     s.d_model_starts.get(), s.nrecords, s.nmodels, s.forward_columns, s.flank, s.boundary ? 1 : 0};
    if (s.nrecords == 0 || s.nmodels == 0) return HAVAC_OK;             // nothing resolves
    chunk = std::min(std::max<uint64_t>(chunk, 1), kMaxWindowChunk);
    for (uint64_t at = 0; at < n; at += chunk) {
        const uint64_t take = std::min(chunk, n - at);
        std::vector<WindowItem> part;
        if (int rc = merge_chunk(err, s, args, d_records + at, take, stream, part)) return rc;
        if (!part.empty()) lists.push_back(std::move(part));
    }
    return HAVAC_OK;
}

WindowBlocks join_window_lists(std::vector<std::vector<WindowItem>>& lists) {
    WindowBlocks out;
    lists.erase(std::remove_if(lists.begin(), lists.end(), [](const std::vector<WindowItem>& l) { return l.empty(); }), lists.end());
    if (lists.size() == 1) {                       // one chunk of one GPU: already the answer
        out.total = lists[0].size();
        out.blocks.push_back(std::move(lists[0]));
        lists.clear();
        return out;
    }
    // a k-way merge by (key, start) through a heap of the lists' heads, with the sweep of havacMergeHitsToWindows on weighted
    // stretches applied as the windows come out; output in blocks of kBlock windows, each input freed once passed
    constexpr size_t kBlock = 1u << 20;
    struct Head { uint64_t key, start; size_t list; };
    auto after = [](const Head& a, const Head& b) { return a.key != b.key ? a.key > b.key : a.start > b.start; };
    std::priority_queue<Head, std::vector<Head>, decltype(after)> heads(after);
    std::vector<size_t> at(lists.size(), 0);
    for (size_t l = 0; l < lists.size(); l++) heads.push(Head{lists[l][0].key, lists[l][0].start, l});
    WindowItem* last = nullptr;
    while (!heads.empty()) {
        const size_t l = heads.top().list;
        heads.pop();
        const WindowItem& w = lists[l][at[l]];
        if (last && last->key == w.key && w.start <= last->end + 1) {
            last->end = std::max(last->end, w.end);
            last->phmm_first = std::min(last->phmm_first, w.phmm_first);
            last->phmm_last = std::max(last->phmm_last, w.phmm_last);
            last->hit_count += w.hit_count;
        } else {
            if (out.blocks.empty() || out.blocks.back().size() == kBlock) {
                out.blocks.emplace_back();
                out.blocks.back().reserve(kBlock);
            }
            out.blocks.back().push_back(w);
            last = &out.blocks.back().back();
            out.total++;
        }
        if (++at[l] < lists[l].size()) heads.push(Head{lists[l][at[l]].key, lists[l][at[l]].start, l});
        else std::vector<WindowItem>().swap(lists[l]);
    }
    lists.clear();
    return out;
}

}  // namespace havac
