// K11: the ratings parser of csrc/textio.hip (tkr_ratings_parse) on the device -- the same four flat arrays, bit for bit, from the
// file's bytes in device memory.
//
//   count      one wave per chunk of chunk_bytes (a power of two): 16 bytes per lane and step, '\n' and ',' counted per 32-bit word,
//              one (lines, commas) pair per chunk
//   scan       one workgroup: exclusive 64-bit prefix of the chunk pairs, totals = (n_lines, n_entries)       -> the host allocates
//   positions  one wave per chunk walks its bytes again: a wave-wide prefix of the per-lane counts gives every delimiter its global
//              index; ',' at p stores the field start p + 1 at its entry index (in item[] / like[], as the low / high word: the
//              fields kernel reads it back before it writes the entry), a line start stores its offset and line_ptr[line]
//   fields     one lane per entry: field end, first and second ':', like = int between them, iid token hashed and looked up
//   lines      one lane per line: strip, uid token = up to the first ',', looked up
//
// Semantics are those stated in textio.hip's header: lines end at '\n' only (a last line without one counts), a line is stripped
// of the six ASCII whitespace bytes at both ends, every ',' opens one field that runs to the next ',' or the stripped end, the iid
// token is the unstripped bytes before the field's first ':', like is the stripped decimal integer (optional sign, saturating at
// +-2,147,483,647) between the first and the second ':' or the field end.  A field without ':' or with another like sets the
// status word to the field's start offset (atomic min: the smallest one wins); the caller turns that into TKR_E_PARSE.
//
// A line or a field may straddle any number of chunks and a chunk may hold no delimiter: the positions pass only needs the counts
// in front of it, and the per-entry / per-line lanes read forward from their start wherever the bytes lie.  No kernel reads a byte
// outside [0, n_bytes): whole 16-byte and 4-byte loads are used only where they lie inside, the tail is read bytewise.
//
// Token lookup: one open-addressing table per id list, laid out on the host (tkr_idtable_build) and uploaded by the caller: slots
// of {offset into the blob, length, index, hash}, length -1 = empty, linear probing from hash & (n_slots - 1).  A hit compares the
// bytes.  The empty token is a key like any other.
//
// The byte helpers, the chunk scan and the workspace layout are shared with K14 (csrc/scan_dev.hip): csrc/text_bytes.h.
#include <string.h>

#include "tkr_common.h"
#include "text_bytes.h"
#include "../../include/tkr.h"

namespace tkr {
namespace {


// FNV-1a over the token's bytes, folded once: the same function lays the table out on the host and probes it on the device
constexpr uint32_t kHashSeed = 2166136261u;
__host__ __device__ inline uint32_t hash_step(uint32_t h, uint32_t byte) { return (h ^ byte) * 16777619u; }
__host__ __device__ inline uint32_t hash_finish(uint32_t h) { return h ^ (h >> 15); }

__device__ __forceinline__ bool is_space(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }      // ' ' \t \n \v \f \r

// (newlines << 16 | commas) of 16 bytes
__device__ __forceinline__ uint32_t count16(const uint32_t (&w)[4]) {
    uint32_t nl = 0, cm = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nl += count_eq(w[k], '\n');
        cm += count_eq(w[k], ',');
    }
    return nl << 16 | cm;
}

__global__ __launch_bounds__(kParseBlock) void parse_count_kernel(Bytes t, int64_t chunk, int64_t n_chunks, uint2* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (kParseBlock / 64) + (threadIdx.x >> 6);
    if (c >= n_chunks) return;                                    // wave-uniform
    const int64_t base = c * chunk;
    const int64_t end = base + chunk < t.n ? base + chunk : t.n;
    uint32_t nl = 0, cm = 0;                                       // per lane at most 16 * chunk / 1024 each
    for (int64_t g = base + lane * 16; g < end; g += kWaveBytes) {
        uint32_t w[4];
        load16(t, g, w);
        const uint32_t v = count16(w);
        nl += v >> 16;
        cm += v & 0xffffu;
    }
    for (int off = 32; off > 0; off >>= 1) {
        nl += __shfl_down(nl, off);
        cm += __shfl_down(cm, off);
    }
    if (lane == 0) counts[c] = make_uint2(nl, cm);
}

__global__ __launch_bounds__(kParseBlock) void parse_positions_kernel(Bytes t, int64_t chunk, int64_t n_chunks,
                                                                     const int64_t* __restrict__ off_nl, const int64_t* __restrict__ off_cm,
                                                                     int64_t n_lines, int64_t n_entries, int64_t* __restrict__ line_start,
                                                                     int64_t* __restrict__ line_ptr, int32_t* __restrict__ item,
                                                                     int32_t* __restrict__ like) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (kParseBlock / 64) + (threadIdx.x >> 6);
    if (c >= n_chunks) return;                                    // wave-uniform
    if (c == 0 && lane == 0) {
        if (n_lines > 0) {
            line_start[0] = 0;
            line_ptr[0] = 0;
        }
        line_ptr[n_lines] = n_entries;
    }
    const int64_t base = c * chunk;
    const int64_t end = base + chunk < t.n ? base + chunk : t.n;
    int64_t run_nl = off_nl[c], run_cm = off_cm[c];                // '\n' and ',' in front of this step
    for (int64_t step = base; step < end; step += kWaveBytes) {    // wave-uniform trip count
        const int64_t g = step + lane * 16;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (g < end) load16(t, g, w);
        const uint32_t own = count16(w);                            // a step holds at most 1024 of either: 16 bits each
        uint32_t incl = own;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, 63);
        if (own) {
            int64_t e = run_cm + ((incl - own) & 0xffffu);          // entry index of this lane's first ','
            int64_t l = run_nl + ((incl - own) >> 16) + 1;          // index of the line that follows this lane's first '\n'
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t b = (w[j >> 2] >> ((j & 3) * 8)) & 0xffu;
                const int64_t next = g + j + 1;
                if (b == ',') {
                    if (e < n_entries) {
                        item[e] = (int32_t)(uint32_t)next;
                        like[e] = (int32_t)(uint32_t)((uint64_t)next >> 32);
                    }
                    ++e;
                } else if (b == '\n') {
                    if (next < t.n && l < n_lines) {
                        line_start[l] = next;
                        line_ptr[l] = e;
                    }
                    ++l;
                }
            }
        }
        run_nl += total >> 16;
        run_cm += total & 0xffffu;
    }
}

struct Table {
    const int4* slots;                                             // {offset into blob, length (-1 = empty), index, hash}
    int64_t n_slots;                                               // a power of two
    Bytes blob;
};

// index of the token text[b, b + len) or -1
__device__ int32_t table_lookup(Cursor& cur, int64_t b, int64_t len, const Table& tb) {
    uint32_t h = kHashSeed;
    for (int64_t i = 0; i < len; ++i) h = hash_step(h, cur.at(b + i));
    h = hash_finish(h);
    const int64_t mask = tb.n_slots - 1;
    int64_t s = h & mask;
    for (int64_t probe = 0; probe < tb.n_slots; ++probe, s = (s + 1) & mask) {
        const int4 sl = tb.slots[s];
        if (sl.y < 0) return -1;
        if ((uint32_t)sl.w != h || (int64_t)sl.y != len || sl.x < 0 || (int64_t)sl.x + len > tb.blob.n) continue;
        Cursor key{tb.blob};
        int64_t i = 0;
        while (i < len && key.at(sl.x + i) == cur.at(b + i)) ++i;
        if (i == len) return sl.z;
    }
    return -1;
}

// textio.hip parse_int on text[b, e)
__device__ bool parse_like(Cursor& cur, int64_t b, int64_t e, int32_t& out) {
    while (b < e && is_space(cur.at(b))) ++b;
    while (e > b && is_space(cur.at(e - 1))) --e;
    if (b == e) return false;
    bool neg = false;
    const uint32_t s = cur.at(b);
    if (s == '+' || s == '-') {
        neg = s == '-';
        ++b;
    }
    if (b == e) return false;
    int64_t v = 0;
    for (; b < e; ++b) {
        const uint32_t d = cur.at(b);
        if (d < '0' || d > '9') return false;
        v = v * 10 + (int64_t)(d - '0');
        if (v > 2147483647LL) v = 2147483647LL;
    }
    out = (int32_t)(neg ? -v : v);
    return true;
}

__global__ __launch_bounds__(kParseBlock) void parse_fields_kernel(Bytes t, Table items, int64_t n_entries, int32_t* __restrict__ item,
                                                                  int32_t* __restrict__ like, unsigned long long* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * kParseBlock;
    for (int64_t e = (int64_t)blockIdx.x * kParseBlock + threadIdx.x; e < n_entries; e += stride) {
        const int64_t q = (int64_t)((uint64_t)(uint32_t)item[e] | (uint64_t)(uint32_t)like[e] << 32);      // the field's start
        int32_t idx = -1, val = 0;
        if (q < 1 || q > t.n) {                                     // not a position the positions pass wrote: counts of another text
            atomicMin(status, 0ull);
        } else {
            Cursor cur{t};
            int64_t p = q, colon = -1, colon2 = -1;
            bool comma = false;
            for (; p < t.n; ++p) {
                const uint32_t b = cur.at(p);
                if (b == ',') { comma = true; break; }
                if (b == '\n') break;
                if (b == ':') {
                    if (colon < 0) colon = p;
                    else if (colon2 < 0) colon2 = p;
                }
            }
            int64_t fe = p;
            if (!comma)                                             // the line's last field ends at the stripped line end
                while (fe > q && is_space(cur.at(fe - 1))) --fe;
            if (colon < 0 || !parse_like(cur, colon + 1, colon2 >= 0 ? colon2 : fe, val)) {
                atomicMin(status, (unsigned long long)q);
                val = 0;
            } else {
                idx = table_lookup(cur, q, colon - q, items);
            }
        }
        item[e] = idx;
        like[e] = val;
    }
}

__global__ __launch_bounds__(kParseBlock) void parse_lines_kernel(Bytes t, Table users, int64_t n_lines, const int64_t* __restrict__ line_start,
                                                                 int32_t* __restrict__ line_user) {
    const int64_t stride = (int64_t)gridDim.x * kParseBlock;
    for (int64_t l = (int64_t)blockIdx.x * kParseBlock + threadIdx.x; l < n_lines; l += stride) {
        int64_t b = line_start[l];
        int32_t idx = -1;
        if (b >= 0 && b < t.n) {
            Cursor cur{t};
            while (b < t.n && cur.at(b) != '\n' && is_space(cur.at(b))) ++b;
            int64_t p = b;
            bool comma = false;
            for (; p < t.n; ++p) {
                const uint32_t c = cur.at(p);
                if (c == ',') { comma = true; break; }
                if (c == '\n') break;
            }
            int64_t ue = p;
            if (!comma)
                while (ue > b && is_space(cur.at(ue - 1))) --ue;
            idx = table_lookup(cur, b, ue - b, users);
        }
        line_user[l] = idx;
    }
}

inline bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
inline bool table_ok(const void* slots, int64_t n_slots, const void* blob, int64_t blob_len) {
    return slots && ((uintptr_t)slots & 15) == 0 && pow2(n_slots) && n_slots <= ((int64_t)1 << 30) && blob_len >= 0 &&
           blob_len <= 2147483647LL && (blob_len == 0 || (blob && ((uintptr_t)blob & 3) == 0));
}

}  // namespace
}  // namespace tkr

extern "C" int64_t tkr_parse_dev_workspace_bytes(int64_t n_bytes, int64_t chunk_bytes) {
    if (n_bytes < 0 || !tkr::chunk_ok(chunk_bytes) || tkr::chunks_of(n_bytes, chunk_bytes) > tkr::kMaxChunks) return TKR_E_INVAL;
    return tkr::Workspace::bytes(tkr::chunks_of(n_bytes, chunk_bytes));
}

extern "C" int64_t tkr_idtable_slots(int64_t n) {
    if (n < 0 || n > ((int64_t)1 << 29)) return TKR_E_INVAL;
    int64_t s = 8;
    while (s < 2 * n) s <<= 1;
    return s;
}

extern "C" int tkr_idtable_build(const char* blob, int64_t blob_len, const int32_t* index, int64_t n, int32_t* slots, int64_t n_slots) {
    if (!slots || n < 0 || blob_len < 0 || blob_len > 2147483647LL || (n > 0 && (!blob || !index)) || !tkr::pow2(n_slots) || n_slots < 8 ||
        n_slots < 2 * n || n_slots > ((int64_t)1 << 30))
        return TKR_E_INVAL;
    for (int64_t s = 0; s < n_slots; ++s) {
        slots[4 * s + 0] = 0;
        slots[4 * s + 1] = -1;
        slots[4 * s + 2] = -1;
        slots[4 * s + 3] = 0;
    }
    const char* p = blob;
    const char* end = blob + blob_len;
    const int64_t mask = n_slots - 1;
    int64_t k = 0;
    while (k < n) {                                                 // n tokens separated by '\n', the last one unterminated (tkr_idmap_create)
        const char* q = blob_len ? static_cast<const char*>(memchr(p, '\n', (size_t)(end - p))) : nullptr;
        if (!q) q = end;
        const int64_t len = q - p;
        uint32_t h = tkr::kHashSeed;
        for (int64_t i = 0; i < len; ++i) h = tkr::hash_step(h, (uint8_t)p[i]);
        h = tkr::hash_finish(h);
        int64_t s = h & mask;
        while (slots[4 * s + 1] >= 0 &&
               !((uint32_t)slots[4 * s + 3] == h && slots[4 * s + 1] == len && memcmp(blob + slots[4 * s + 0], p, (size_t)len) == 0))
            s = (s + 1) & mask;                                     // at most half the slots are taken: an empty one comes
        slots[4 * s + 0] = (int32_t)(p - blob);
        slots[4 * s + 1] = (int32_t)len;
        slots[4 * s + 2] = index[k++];                              // a token listed twice keeps its last index, as the host map does
        slots[4 * s + 3] = (int32_t)h;
        if (q == end) break;
        p = q + 1;
    }
    return k == n ? TKR_OK : TKR_E_INVAL;
}

extern "C" int tkr_ratings_count_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                                     int64_t* totals_out, void* stream) {
    if (n_bytes < 0 || !tkr::chunk_ok(chunk_bytes) || !workspace || !totals_out || (n_bytes > 0 && !text) || ((uintptr_t)text & 15) ||
        ((uintptr_t)workspace & 15))
        return TKR_E_INVAL;
    const int64_t n_chunks = tkr::chunks_of(n_bytes, chunk_bytes);
    if (n_chunks > tkr::kMaxChunks || workspace_bytes < tkr::Workspace::bytes(n_chunks)) return TKR_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_bytes == 0) {                                             // zero lines, zero entries
        TKR_CHECK(hipMemsetAsync(totals_out, 0, 2 * sizeof(int64_t), s));
        return TKR_OK;
    }
    const tkr::Bytes t{static_cast<const uint8_t*>(text), n_bytes};
    const tkr::Workspace ws(workspace, n_chunks);
    const unsigned blocks = (unsigned)((n_chunks + tkr::kParseBlock / 64 - 1) / (tkr::kParseBlock / 64));
    hipLaunchKernelGGL(tkr::parse_count_kernel, dim3(blocks), dim3(tkr::kParseBlock), 0, s, t, chunk_bytes, n_chunks, ws.counts);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tkr::chunk_scan_kernel, dim3(1), dim3(tkr::kScanThreads), 0, s, t, ws.counts, n_chunks, ws.off_x, ws.off_y, totals_out);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_ratings_emit_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                                    int64_t n_lines, int64_t n_entries, const int32_t* user_slots, int64_t user_n_slots,
                                    const void* user_blob, int64_t user_blob_len, const int32_t* item_slots, int64_t item_n_slots,
                                    const void* item_blob, int64_t item_blob_len, int64_t* line_start, int32_t* line_user,
                                    int64_t* line_ptr, int32_t* item, int32_t* like, int64_t* status, void* stream) {
    if (n_bytes < 0 || !tkr::chunk_ok(chunk_bytes) || !workspace || (n_bytes > 0 && !text) || ((uintptr_t)text & 15) ||
        ((uintptr_t)workspace & 15) || n_lines < 0 || n_entries < 0 || n_lines > n_bytes || n_entries > n_bytes || !line_ptr || !status ||
        (n_lines > 0 && (!line_start || !line_user)) || (n_entries > 0 && (!item || !like)) ||
        !tkr::table_ok(user_slots, user_n_slots, user_blob, user_blob_len) || !tkr::table_ok(item_slots, item_n_slots, item_blob, item_blob_len))
        return TKR_E_INVAL;
    const int64_t n_chunks = tkr::chunks_of(n_bytes, chunk_bytes);
    if (n_chunks > tkr::kMaxChunks || workspace_bytes < tkr::Workspace::bytes(n_chunks)) return TKR_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    TKR_CHECK(hipMemsetAsync(status, 0xff, sizeof(int64_t), s));    // -1: no malformed field
    if (n_bytes == 0) {
        TKR_CHECK(hipMemsetAsync(line_ptr, 0, sizeof(int64_t), s));
        return TKR_OK;
    }
    const tkr::Bytes t{static_cast<const uint8_t*>(text), n_bytes};
    const tkr::Workspace ws(workspace, n_chunks);
    const tkr::Table users{reinterpret_cast<const int4*>(user_slots), user_n_slots, {static_cast<const uint8_t*>(user_blob), user_blob_len}};
    const tkr::Table items{reinterpret_cast<const int4*>(item_slots), item_n_slots, {static_cast<const uint8_t*>(item_blob), item_blob_len}};
    const unsigned blocks = (unsigned)((n_chunks + tkr::kParseBlock / 64 - 1) / (tkr::kParseBlock / 64));
    hipLaunchKernelGGL(tkr::parse_positions_kernel, dim3(blocks), dim3(tkr::kParseBlock), 0, s, t, chunk_bytes, n_chunks, ws.off_x, ws.off_y,
                       n_lines, n_entries, line_start, line_ptr, item, like);
    TKR_LAUNCH_CHECK();
    if (n_entries > 0) {
        hipLaunchKernelGGL(tkr::parse_fields_kernel, dim3(tkr::lane_grid(n_entries)), dim3(tkr::kParseBlock), 0, s, t, items, n_entries, item,
                           like, reinterpret_cast<unsigned long long*>(status));
        TKR_LAUNCH_CHECK();
    }
    if (n_lines > 0) {
        hipLaunchKernelGGL(tkr::parse_lines_kernel, dim3(tkr::lane_grid(n_lines)), dim3(tkr::kParseBlock), 0, s, t, users, n_lines, line_start,
                           line_user);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}
