// K14: one matrix token -> fp32, the arithmetic of strtod followed by (float) for the tokens it can be done for exactly with
// 64-bit integers.  The same code runs on the device (csrc/scan_dev.hip, one lane per token) and on the host
// (tkr_matrix_token_host), over any reader with `uint32_t at(int64_t i)`.
//
// A token is PLAIN when it is [+-]? digits* ('.' digits*)? with at least one digit, at most 19 digits from its first non-zero
// digit to its last digit (w, their integer value, is below 10^19 < 2^64) and at most 19 digits f behind the '.' (10^f < 2^64).
// Its value w / 10^f is 0 or lies in [1e-19, 1e19): no subnormal, no overflow.  It is rounded TWICE, as the host reader does:
// to 53 bits (the double strtod returns), then to 24 bits (the narrowing cast), both to nearest even.  Every other token is
// HARD and left to the host's strtod: exponent forms, inf, nan, hex floats, longer digit strings, garbage.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TKR_HD __host__ __device__ inline
#else
#define TKR_HD inline
#endif

namespace tkr {

constexpr int kScanMaxDigits = 19;

TKR_HD int scan_clz64(uint64_t v) {                                // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}

// w / 10^f, w != 0, both as stated above -> the bits of the fp32 (sign clear)
TKR_HD uint32_t scan_ratio_bits(uint64_t w, int f) {
    uint64_t d = 1;
    for (int k = 0; k < f; ++k) d *= 10u;
    const int lw = scan_clz64(w), ld = scan_clz64(d);
    const uint64_t wn = w << lw, dn = d << ld;                      // both in [2^63, 2^64): wn / dn lies in (1/2, 2)
    // q = floor(wn * 2^(63 or 64) / dn) with exactly 64 significant bits, by restoring division: r < dn throughout, the dividend's
    // low word is shifted in from the top (all zeros but, for wn >= dn, the bit that wn >> 1 dropped)
    const bool ge = wn >= dn;
    uint64_t r = ge ? wn >> 1 : wn;
    uint64_t low = ge ? (wn & 1u) << 63 : 0u;
    uint64_t q = 0;
    for (int k = 0; k < 64; ++k) {
        const uint64_t carry = r >> 63;
        r = (r << 1) | (low >> 63);
        low <<= 1;
        q <<= 1;
        if (carry || r >= dn) {
            r -= dn;
            q |= 1u;
        }
    }
    // value = (q + r / dn) * 2^e, 2^63 <= q < 2^64
    int e = ld - lw - (ge ? 63 : 64);
    // first rounding: 64 -> 53 bits, the remainder of the division is the sticky bit
    uint64_t m = q >> 11;
    const uint64_t rest = q & 0x7ffu;
    if (rest > 0x400u || (rest == 0x400u && (r != 0 || (m & 1u)))) ++m;
    if (m >> 53) {                                                   // 2^53: one bit longer, the low bit is 0
        m >>= 1;
        ++e;
    }
    // second rounding: 53 -> 24 bits of the double, which is exact now
    uint32_t m24 = (uint32_t)(m >> 29);
    const uint32_t rest2 = (uint32_t)m & 0x1fffffffu;
    if (rest2 > 0x10000000u || (rest2 == 0x10000000u && (m24 & 1u))) ++m24;
    if (m24 >> 24) {
        m24 >>= 1;
        ++e;
    }
    // value = m24 * 2^(e + 40) = 1.xxx * 2^(e + 63): exponents -64 ... 63, all normal
    return (uint32_t)(e + 63 + 127) << 23 | (m24 & 0x7fffffu);
}

// the token that starts at text[b]: it ends at the first ' ' or '\n' at or after b, or at `limit`.
// -> 1: plain, *bits = its fp32; 0: hard, *bits = 0.  *used = the bytes read as part of the token (its length when it is plain)
template <class Reader>
TKR_HD int scan_token(Reader& text, int64_t b, int64_t limit, uint32_t* bits, int64_t* used) {
    int64_t i = b;
    uint32_t sign = 0;
    if (i < limit) {
        const uint32_t c = text.at(i);
        if (c == '+' || c == '-') {
            sign = c == '-' ? 0x80000000u : 0u;
            ++i;
        }
    }
    uint64_t w = 0;
    int sig = 0, f = 0;
    bool digit = false, dot = false, hard = false;
    for (; i < limit; ++i) {
        const uint32_t c = text.at(i);
        if (c == ' ' || c == '\n') break;
        if (c >= '0' && c <= '9') {
            digit = true;
            if (dot && f <= kScanMaxDigits) ++f;
            if (sig > 0 || c != '0') {
                if (sig < kScanMaxDigits) w = w * 10u + (c - '0');
                if (sig <= kScanMaxDigits) ++sig;
            }
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            hard = true;
            break;
        }
    }
    *used = i - b;
    *bits = 0;
    if (hard || !digit || sig > kScanMaxDigits || f > kScanMaxDigits) return 0;
    *bits = sign | (w ? scan_ratio_bits(w, f) : 0u);
    return 1;
}

}  // namespace tkr
