"""'%f' of an fp32 value with integers only: the readable statement of what csrc/format_dev.hip computes (K13).

    x = +-m * 2^ex, m < 2^24: exponent field 0 -> ex = -149, m = the fraction bits; else ex = e - 150, m carries the hidden bit
    ex >= 0   the integer m << ex, fraction 000000; from 2^64 on its decimal digits come from four 32-bit limbs divided by 10^9
              five times (chunks of nine digits, least significant first)
    ex < 0    sh = -ex: integer part m >> sh, fraction ((m mod 2^sh) * 10^6) >> sh, rounded half to even on the remainder; a fraction
              that reaches 10^6 carries into the integer part; sh >= 64: the fraction is 0 and never a tie
    a set sign bit prints '-' (-0.000000 included), +-inf prints inf / -inf, every NaN prints nan
"""
import struct

import numpy as np

EDGE_BITS = [
    0x00000000,                                       # 0
    0x00000001, 0x007fffff,                           # smallest and largest denormal
    0x7f800000,                                       # inf
    0x7fc00000, 0x7f800001, 0x7fc12345, 0x7fffffff,   # NaNs without and with payload
    0x7f7fffff,                                       # FLT_MAX
    0x4b000000, 0x4b800000,                           # 2^23, 2^24
    0x5f000000, 0x5f7fffff, 0x5f800000,               # 2^63, the fp32 just below 2^64, 2^64
    0x6f800000, 0x7f000000,                           # 2^96, 2^127
    0x3f7fffff, 0x411fffff,                           # the largest fp32 below 1 and below 10
]


def bits_of(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


def edge_bits():
    """the values the issue lists (bit patterns), each with its negative"""
    bits = list(EDGE_BITS)
    for j in range(1, 128, 2):                        # ties of the sixth digit: j / 128 = 0.xxxxxx5 exactly, also behind 1 and 1023
        for add in (0, 1, 1023):
            bits.append(bits_of(j / 128.0 + add))
    bits += [bits_of(1.5 * 2.0 ** -20), bits_of(999999.94), bits_of(0.9999995), bits_of(1e-9)]
    return np.array(bits + [b | 0x80000000 for b in bits], dtype=np.uint32)


def _big_digits(m, ex):
    """decimal digits of m << ex (41 <= ex <= 104) through four 32-bit limbs"""
    v = m << ex
    limbs = [(v >> (32 * k)) & 0xffffffff for k in range(4)]
    chunks = []
    for _ in range(5):
        rem = 0
        for k in (3, 2, 1, 0):
            cur = rem << 32 | limbs[k]
            limbs[k], rem = cur // 10 ** 9, cur % 10 ** 9
        chunks.append(rem)
    top = max(k for k in range(5) if chunks[k])
    return str(chunks[top]) + ''.join('%09d' % chunks[k] for k in range(top - 1, -1, -1))


def format_f32(bits):
    """the text of '%f' % float(x) for the fp32 with these 32 bits"""
    bits = int(bits)
    e, f = (bits >> 23) & 0xff, bits & 0x7fffff
    sign = '-' if bits >> 31 else ''
    if e == 255:
        return 'nan' if f else sign + 'inf'
    m, ex = (f | 0x800000, e - 150) if e else (f, -149)
    if ex >= 0:
        return sign + (str(m << ex) if ex <= 40 else _big_digits(m, ex)) + '.000000'
    sh = -ex
    if sh >= 64:
        return sign + '0.000000'
    ip, p = m >> sh, (m & ((1 << sh) - 1)) * 10 ** 6
    frac, r, half = p >> sh, p & ((1 << sh) - 1), 1 << (sh - 1)
    if r > half or (r == half and frac & 1):
        frac += 1
    if frac == 10 ** 6:
        frac, ip = 0, ip + 1
    return '%s%d.%06d' % (sign, ip, frac)


def python_f(bits):
    """what the writers are held to: Python's own '%f', 'nan' for either sign of NaN"""
    x = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
    return 'nan' if x != x else '%f' % x
