// K14: the matrix reader of csrc/textio.hip (tkr_matrix_read) on the device -- the same fp32 array, bit for bit, from the file's
// bytes in device memory.  The device decides nothing about malformed input: it establishes that the file has the CANONICAL layout
// (below), converts the PLAIN tokens exactly (csrc/scan_num.h) and marks the others HARD for the host's strtod.  Any other file is
// reported as not canonical and read by the host reader as a whole.
//
//   count      one wave per chunk of chunk_bytes (a power of two): 16 bytes per lane and step; '\n' and token starts counted per
//              32-bit word, the layout rules checked on the same marks; one (lines, tokens) pair per chunk
//   scan       one workgroup: exclusive 64-bit prefix of the chunk pairs, totals = (n_lines, n_tokens, layout status)  -> the host allocates
//   positions  one wave per chunk walks its bytes again: a wave-wide prefix of the per-lane counts gives every token start its global
//              index, its offset goes to tok_start[index]; every line start checks that its first token has index line * cols
//   convert    one lane per token: byte walk, classify, convert (scan_num.h), store the float; a wave ballot stores the 64 hard bits
//   hard count one workgroup sums the popcounts of the hard words
//
// Canonical: none of \t \r \v \f anywhere; the first byte is a token byte (anything but ' ' and '\n'); none of the pairs "  ",
// "\n ", "\n\n"; every line has as many tokens as the first.  Then a token starts at p when byte[p] is a token byte and p == 0 or
// byte[p - 1] is ' ' or '\n', and runs to the next ' ' or '\n' or the end of the text: the host's tokenisation exactly (lines end
// at '\n', a last line without one counts, a line is stripped at both ends, tokens are split on ' ').  The status word holds the
// smallest offset that breaks a rule (the second byte of a pair; for a ragged file the start of the first line whose first token
// is not token line * cols, or n_bytes when only the last line's length differs), -1 when none does.
//
// A token or a line may straddle any number of chunks and a chunk may hold no delimiter.  The byte in front of a lane's 16 is read
// from memory (never at offset -1: the text's first byte is treated as following a '\n').  No kernel reads a byte outside
// [0, n_bytes).  The only atomic is the status word's atomic min; everything else is a plain store to its own place: deterministic.
#include <string.h>

#include "tkr_common.h"
#include "text_bytes.h"
#include "scan_num.h"
#include "../../include/tkr.h"

namespace tkr {
namespace {

// what the 16 bytes [g, g + 16) of a lane hold, as bit 7 of the byte's place in its word
struct Marks {
    uint32_t nl[4];                                                // '\n'
    uint32_t start[4];                                             // a token starts here
    uint32_t line[4];                                              // a line starts here (the byte in front is '\n', or this is byte 0)
    uint32_t bad[4];                                               // breaks a layout rule
};

__device__ __forceinline__ Marks mark16(const Bytes& t, int64_t g, const uint32_t (&w)[4]) {
    const uint32_t before = g > 0 ? (uint32_t)t.p[g - 1] : (uint32_t)'\n';
    uint32_t carry_sp = before == ' ' ? 0x80u : 0u, carry_nl = before == '\n' ? 0x80u : 0u;
    Marks m;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t left = t.n - (g + 4 * k);                     // bytes of this word inside the text
        const uint32_t valid = left >= 4 ? 0x80808080u : left <= 0 ? 0u : 0x80808080u & ((1u << (8 * (int)left)) - 1u);
        const uint32_t sp = mark_eq(w[k], ' '), nl = mark_eq(w[k], '\n');
        const uint32_t other = mark_eq(w[k], '\t') | mark_eq(w[k], '\r') | mark_eq(w[k], '\v') | mark_eq(w[k], '\f');
        const uint32_t prev_sp = sp << 8 | carry_sp, prev_nl = nl << 8 | carry_nl;
        m.nl[k] = nl & valid;
        m.start[k] = ~(sp | nl) & (prev_sp | prev_nl) & valid;
        m.line[k] = prev_nl & valid;
        m.bad[k] = (other | (sp & (prev_sp | prev_nl)) | (nl & prev_nl)) & valid;
        carry_sp = sp >> 24;                                        // bit 31 -> bit 7
        carry_nl = nl >> 24;
    }
    return m;
}

__global__ __launch_bounds__(kParseBlock) void scan_count_kernel(Bytes t, int64_t chunk, int64_t n_chunks, uint2* __restrict__ counts,
                                                                unsigned long long* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (kParseBlock / 64) + (threadIdx.x >> 6);
    if (c >= n_chunks) return;                                    // wave-uniform
    const int64_t base = c * chunk;
    const int64_t end = base + chunk < t.n ? base + chunk : t.n;
    uint32_t nl = 0, tk = 0;                                       // per lane at most 16 * chunk / 1024 each
    int64_t first_bad = -1;
    for (int64_t g = base + lane * 16; g < end; g += kWaveBytes) {
        uint32_t w[4];
        load16(t, g, w);
        const Marks m = mark16(t, g, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nl += __popc(m.nl[k]);
            tk += __popc(m.start[k]);
            if (m.bad[k] && first_bad < 0) first_bad = g + 4 * k + ((__ffs(m.bad[k]) - 1) >> 3);
        }
    }
    if (first_bad >= 0) atomicMin(status, (unsigned long long)first_bad);
    for (int off = 32; off > 0; off >>= 1) {
        nl += __shfl_down(nl, off);
        tk += __shfl_down(tk, off);
    }
    if (lane == 0) counts[c] = make_uint2(nl, tk);
}

__global__ void scan_status_kernel(const unsigned long long* __restrict__ status, int64_t* __restrict__ totals) {
    totals[2] = (int64_t)*status;
}

__global__ __launch_bounds__(kParseBlock) void scan_positions_kernel(Bytes t, int64_t chunk, int64_t n_chunks,
                                                                    const int64_t* __restrict__ off_nl, const int64_t* __restrict__ off_tk,
                                                                    int64_t n_lines, int64_t n_tokens, int64_t cols,
                                                                    int64_t* __restrict__ tok_start, unsigned long long* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (kParseBlock / 64) + (threadIdx.x >> 6);
    if (c >= n_chunks) return;                                    // wave-uniform
    if (c == 0 && lane == 0 && (__umul64hi((uint64_t)n_lines, (uint64_t)cols) != 0 || (uint64_t)n_lines * (uint64_t)cols != (uint64_t)n_tokens))
        atomicMin(status, (unsigned long long)t.n);                // every line may start where it should and the last one still differ
    const int64_t base = c * chunk;
    const int64_t end = base + chunk < t.n ? base + chunk : t.n;
    int64_t run_nl = off_nl[c], run_tk = off_tk[c];                // '\n' and token starts in front of this step
    for (int64_t step = base; step < end; step += kWaveBytes) {    // wave-uniform trip count
        const int64_t g = step + lane * 16;
        uint32_t own = 0;
        Marks m;
        if (g < end) {
            uint32_t w[4];
            load16(t, g, w);
            m = mark16(t, g, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) own += __popc(m.nl[k]) << 16 | __popc(m.start[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) m.nl[k] = m.start[k] = m.line[k] = m.bad[k] = 0u;
        }
        uint32_t incl = own;                                        // a step holds at most 1024 of either: 16 bits each
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, 63);
        if (g < end) {
            int64_t k_tok = run_tk + ((incl - own) & 0xffffu);      // index of this lane's first token start
            int64_t k_line = run_nl + ((incl - own) >> 16);         // '\n' in front of this lane's first byte = the line it lies in
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int bit = (j & 3) * 8 + 7;
                if ((m.line[j >> 2] >> bit) & 1u) {                 // the line's first token is the next start: k_tok
                    const uint64_t want = (uint64_t)k_line * (uint64_t)cols;
                    if (__umul64hi((uint64_t)k_line, (uint64_t)cols) != 0 || want != (uint64_t)k_tok || !((m.start[j >> 2] >> bit) & 1u))
                        atomicMin(status, (unsigned long long)(g + j));
                }
                if ((m.start[j >> 2] >> bit) & 1u) {
                    if (k_tok < n_tokens) tok_start[k_tok] = g + j;
                    ++k_tok;
                }
                if ((m.nl[j >> 2] >> bit) & 1u) ++k_line;
            }
        }
        run_nl += total >> 16;
        run_tk += total & 0xffffu;
    }
}

__global__ __launch_bounds__(kParseBlock) void scan_convert_kernel(Bytes t, int64_t n_tokens, const int64_t* __restrict__ tok_start,
                                                                  uint32_t* __restrict__ data, unsigned long long* __restrict__ hard,
                                                                  unsigned long long* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * kParseBlock;       // a multiple of 64: a wave's tokens share one word of `hard`
    for (int64_t first = (int64_t)blockIdx.x * kParseBlock + (threadIdx.x & ~63); first < n_tokens; first += stride) {      // wave-uniform
        const int64_t i = first + (threadIdx.x & 63);
        bool is_hard = false;
        if (i < n_tokens) {
            const int64_t b = tok_start[i];
            uint32_t bits = 0;
            if (b < 0 || b >= t.n) {                                // not a position the positions pass wrote: counts of another text
                atomicMin(status, 0ull);
            } else {
                Cursor cur{t};
                int64_t used;
                is_hard = !scan_token(cur, b, t.n, &bits, &used);
            }
            data[i] = bits;
        }
        const unsigned long long mask = __ballot(is_hard);
        if ((threadIdx.x & 63) == 0) hard[first >> 6] = mask;
    }
}

__global__ __launch_bounds__(kScanThreads) void scan_hard_count_kernel(const unsigned long long* __restrict__ hard, int64_t n_words,
                                                                      int64_t* __restrict__ counts) {
    __shared__ int64_t s[kScanThreads];
    int64_t n = 0;
    for (int64_t k = threadIdx.x; k < n_words; k += kScanThreads) n += __popcll(hard[k]);
    s[threadIdx.x] = n;
    __syncthreads();
    for (int d = kScanThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[1] = s[0];
}

struct HostBytes {
    const char* p;
    uint32_t at(int64_t i) const { return (uint8_t)p[i]; }
};

}  // namespace
}  // namespace tkr

extern "C" int64_t tkr_scan_dev_workspace_bytes(int64_t n_bytes, int64_t chunk_bytes) {
    if (n_bytes < 0 || !tkr::chunk_ok(chunk_bytes) || tkr::chunks_of(n_bytes, chunk_bytes) > tkr::kMaxChunks) return TKR_E_INVAL;
    return tkr::Workspace::bytes(tkr::chunks_of(n_bytes, chunk_bytes));
}

extern "C" int tkr_matrix_token_host(const char* tok, int64_t len, float* out) {
    if (!tok || len < 0 || !out) return TKR_E_INVAL;
    tkr::HostBytes text{tok};
    uint32_t bits = 0;
    int64_t used = 0;
    if (!tkr::scan_token(text, 0, len, &bits, &used) || used != len) return 0;      // a ' ' or '\n' inside: no token of a matrix
    memcpy(out, &bits, sizeof(bits));
    return 1;
}

extern "C" int tkr_matrix_count_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                                    int64_t* totals_out, void* stream) {
    if (n_bytes < 0 || !tkr::chunk_ok(chunk_bytes) || !workspace || !totals_out || (n_bytes > 0 && !text) || ((uintptr_t)text & 15) ||
        ((uintptr_t)workspace & 15) || ((uintptr_t)totals_out & 7))
        return TKR_E_INVAL;
    const int64_t n_chunks = tkr::chunks_of(n_bytes, chunk_bytes);
    if (n_chunks > tkr::kMaxChunks || workspace_bytes < tkr::Workspace::bytes(n_chunks)) return TKR_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_bytes == 0) {                                             // the empty file is canonical: zero lines, zero tokens, status -1
        TKR_CHECK(hipMemsetAsync(totals_out, 0, 2 * sizeof(int64_t), s));
        TKR_CHECK(hipMemsetAsync(totals_out + 2, 0xff, sizeof(int64_t), s));
        return TKR_OK;
    }
    const tkr::Bytes t{static_cast<const uint8_t*>(text), n_bytes};
    const tkr::Workspace ws(workspace, n_chunks);
    TKR_CHECK(hipMemsetAsync(ws.spare, 0xff, sizeof(unsigned long long), s));       // -1: no rule broken
    const unsigned blocks = (unsigned)((n_chunks + tkr::kParseBlock / 64 - 1) / (tkr::kParseBlock / 64));
    hipLaunchKernelGGL(tkr::scan_count_kernel, dim3(blocks), dim3(tkr::kParseBlock), 0, s, t, chunk_bytes, n_chunks, ws.counts, ws.spare);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tkr::chunk_scan_kernel, dim3(1), dim3(tkr::kScanThreads), 0, s, t, ws.counts, n_chunks, ws.off_x, ws.off_y, totals_out);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tkr::scan_status_kernel, dim3(1), dim3(1), 0, s, ws.spare, totals_out);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_matrix_emit_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                                   int64_t n_lines, int64_t n_tokens, int64_t cols, int64_t* tok_start, float* data, uint64_t* hard,
                                   int64_t* counts, void* stream) {
    if (n_bytes < 0 || !tkr::chunk_ok(chunk_bytes) || !workspace || (n_bytes > 0 && !text) || ((uintptr_t)text & 15) ||
        ((uintptr_t)workspace & 15) || n_lines < 0 || n_tokens < 0 || cols < 0 || n_lines > n_bytes || n_tokens > n_bytes || cols > n_bytes ||
        !counts || ((uintptr_t)counts & 7) || (n_tokens > 0 && (!tok_start || !data || !hard)) || ((uintptr_t)tok_start & 7) ||
        ((uintptr_t)data & 3) || ((uintptr_t)hard & 7))
        return TKR_E_INVAL;
    const int64_t n_chunks = tkr::chunks_of(n_bytes, chunk_bytes);
    if (n_chunks > tkr::kMaxChunks || workspace_bytes < tkr::Workspace::bytes(n_chunks)) return TKR_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    TKR_CHECK(hipMemsetAsync(counts, 0xff, sizeof(int64_t), s));    // -1: canonical
    TKR_CHECK(hipMemsetAsync(counts + 1, 0, sizeof(int64_t), s));   // no hard token
    if (n_bytes == 0) return TKR_OK;
    const tkr::Bytes t{static_cast<const uint8_t*>(text), n_bytes};
    const tkr::Workspace ws(workspace, n_chunks);
    unsigned long long* status = reinterpret_cast<unsigned long long*>(counts);
    const unsigned blocks = (unsigned)((n_chunks + tkr::kParseBlock / 64 - 1) / (tkr::kParseBlock / 64));
    hipLaunchKernelGGL(tkr::scan_positions_kernel, dim3(blocks), dim3(tkr::kParseBlock), 0, s, t, chunk_bytes, n_chunks, ws.off_x, ws.off_y,
                       n_lines, n_tokens, cols, tok_start, status);
    TKR_LAUNCH_CHECK();
    if (n_tokens > 0) {
        hipLaunchKernelGGL(tkr::scan_convert_kernel, dim3(tkr::lane_grid(n_tokens)), dim3(tkr::kParseBlock), 0, s, t, n_tokens, tok_start,
                           reinterpret_cast<uint32_t*>(data), reinterpret_cast<unsigned long long*>(hard), status);
        TKR_LAUNCH_CHECK();
        hipLaunchKernelGGL(tkr::scan_hard_count_kernel, dim3(1), dim3(tkr::kScanThreads), 0, s, reinterpret_cast<unsigned long long*>(hard),
                           (n_tokens + 63) / 64, counts);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}
