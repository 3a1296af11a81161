// SD file records of ligand poses, formatted on the device (pd_sdf_format; physdock_amd/sdfio.py builds the tables, tests/sdf_ref.py is
// the written definition).  The format is the CTfile V2000 specification, not RDKit's bytes.
//
// Record r of a call shows pose p = order[r] (order == nullptr: p = r) and is, byte for byte,
//   * the molblock: the M bytes of `tmpl` (title, program line, comment, counts line, atom lines with 30 blank coordinate columns, bond
//     lines, M  CHG lines, M  END, every line with its newline), where map[i] < 0 copies tmpl[i] and map[i] = 30 s + col fills column col
//     (0 .. 29) of template atom s: character col % 10 of f"{v:10.4f}" of v = x[p, atom[s], col / 10];
//   * for item k = 0 .. K-1: the header bytes hdr[hdr_start[k] .. hdr_start[k + 1]) (">  <name>\n"), the value's text, "\n\n";
//   * "$$$$\n".
// A value is the 32 bits values[k, p]: decimals[k] = d in 0 .. 8 reads them as a float32 and prints f"{v:.{d}f}" as Python does (no
// padding; "-0.0000", "nan", "inf", "-inf"), decimals[k] < 0 reads them as an int32 and prints str(v).
//
// Numbers are exact: for a float32 v and d <= 8 the product |v| 10^d is exact in float64 (24 significand bits and at most 19 for 5^8),
// so rint of it is the round-half-even of the correctly rounded decimal conversion, and every digit is then taken from that integer.
// The sign survives rounding to zero.  A coordinate that is not finite or does not fit its 10 columns (after rounding above
// 99999.9999 or below -9999.9999) is counted in *overflow and filled with '*'; a value with |v| 10^d >= 1e15 is counted and written
// as a single '*'; a record whose order[r] is outside 0 .. P-1 is written from pose 0 with every number of it counted.  *overflow is
// the caller's to zero and to read.
//
// The host passes `fixed` (the bytes of a record that are not a value's text: M, the headers with the two newlines behind each value,
// "$$$$\n"), `longest` (fixed + the longest text of every value: 18 characters for a float32 - sign, 16 digits, the point -, 11 for an
// int32) and `capacity` >= n * longest, the bytes of `out`; nothing is written at or behind out[capacity].
//
// Three launches on the caller's stream, no atomics but the overflow counter:
//   measure  one thread per (record, item): the length of the value's text -> vlen uint8 [n,K]            (skipped when K = 0)
//   offsets  one block: record length = fixed + sum of its vlen; exclusive scan over the n records in int64, in chunks of the block
//            size with a carry -> offsets int64 [n + 1]
//   write    one thread per byte of a record on a grid of (blocks per longest possible record, n); threads past the record leave
#include "common.h"
#include "physdock_hip.h"

namespace {

constexpr int SDF_BLOCK = 256;
constexpr int SDF_MAX_ITEMS = 32;

__device__ __forceinline__ unsigned long long sdf_pow10(int e) {         // e = 0 .. 16
    unsigned long long p = 1;
    for (int k = 0; k < e; ++k) p *= 10ull;
    return p;
}

__device__ __forceinline__ int sdf_digits(unsigned long long m) {         // decimal digits of m, 1 for m = 0
    int n = 1;
    while (m >= 10ull) { m /= 10ull; ++n; }
    return n;
}

// The text of one value as a number to take digits from.  kind: 0 digits of m (D of them, zero-padded on the left, a point in front of
// the last d when d > 0, '-' in front when neg), 1 "nan", 2 "inf" / "-inf", 3 "*" (counted by the caller).
struct SdfNumber { unsigned long long m; int D, d, kind; bool neg; };

__device__ __forceinline__ SdfNumber sdf_number(int bits, int dec) {
    SdfNumber r;
    r.kind = 0;
    if (dec < 0) {
        r.neg = bits < 0;
        const long long w = bits;
        r.m = (unsigned long long)(r.neg ? -w : w);
        r.d = 0;
        r.D = sdf_digits(r.m);
        return r;
    }
    const float v = __int_as_float(bits);
    r.neg = __builtin_signbit(v);
    r.d = dec;
    r.m = 0;
    r.D = 1;
    if (v != v) { r.kind = 1; r.neg = false; return r; }
    if (__builtin_isinf(v)) { r.kind = 2; return r; }
    const double sc = fabs((double)v) * (double)sdf_pow10(dec);
    if (!(sc < 1e15)) { r.kind = 3; r.neg = false; return r; }
    r.m = (unsigned long long)rint(sc);
    const int nd = sdf_digits(r.m);
    r.D = nd > dec + 1 ? nd : dec + 1;
    return r;
}

__device__ __forceinline__ int sdf_length(const SdfNumber& r) {
    if (r.kind == 1) return 3;
    if (r.kind == 2) return r.neg ? 4 : 3;
    if (r.kind == 3) return 1;
    return (r.neg ? 1 : 0) + r.D + (r.d > 0 ? 1 : 0);
}

__device__ __forceinline__ unsigned char sdf_char(const SdfNumber& r, int q) {      // character q of the text, q < sdf_length(r)
    if (r.kind == 1) return q == 1 ? 'a' : 'n';
    if (r.kind == 3) return '*';
    if (r.neg) {
        if (q == 0) return '-';
        --q;
    }
    if (r.kind == 2) return q == 0 ? 'i' : q == 1 ? 'n' : 'f';
    const int point = r.D - r.d;                                         // the digits in front of the point
    if (r.d > 0 && q == point) return '.';
    const int j = q < point ? q : q - 1;
    return (unsigned char)('0' + (int)((r.m / sdf_pow10(r.D - 1 - j)) % 10ull));
}

__device__ __forceinline__ int sdf_pose(const int* __restrict__ order, int r, int P, bool* ok) {
    const int p = order ? order[r] : r;
    *ok = p >= 0 && p < P;
    return *ok ? p : 0;
}

__global__ __launch_bounds__(SDF_BLOCK) void sdf_measure_kernel(const int* __restrict__ values, const int* __restrict__ decimals,
                                                                const int* __restrict__ order, unsigned char* __restrict__ vlen,
                                                                int* __restrict__ overflow, int n, int P, int K) {
    const long long idx = (long long)blockIdx.x * SDF_BLOCK + threadIdx.x;
    if (idx >= (long long)n * K) return;
    const int r = (int)(idx / K), k = (int)(idx - (long long)r * K);
    bool ok;
    const int p = sdf_pose(order, r, P, &ok);
    const SdfNumber num = sdf_number(values[(long long)k * P + p], decimals[k]);
    if (num.kind == 3 || !ok) atomicAdd(overflow, 1);
    vlen[idx] = (unsigned char)sdf_length(num);
}

__global__ __launch_bounds__(SDF_BLOCK) void sdf_offsets_kernel(const unsigned char* __restrict__ vlen, long long* __restrict__ offsets,
                                                                long long fixed, int n, int K) {
    __shared__ long long s[SDF_BLOCK];
    const int t = threadIdx.x;
    long long carry = 0;                                                 // the same in every thread
    for (int base = 0; base < n; base += SDF_BLOCK) {
        const int r = base + t;
        long long len = 0;
        if (r < n) {
            len = fixed;
            for (int k = 0; k < K; ++k) len += vlen[(long long)r * K + k];
        }
        s[t] = len;
        __syncthreads();
        for (int o = 1; o < SDF_BLOCK; o <<= 1) {                        // inclusive scan of the chunk
            const long long add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        if (r < n) offsets[r] = carry + s[t] - len;
        carry += s[SDF_BLOCK - 1];
        __syncthreads();
    }
    if (t == 0) offsets[n] = carry;
}

__global__ __launch_bounds__(SDF_BLOCK) void sdf_write_kernel(const float* __restrict__ x, const unsigned char* __restrict__ tmpl,
                                                              const int* __restrict__ map, const int* __restrict__ atom,
                                                              const int* __restrict__ order, const unsigned char* __restrict__ hdr,
                                                              const int* __restrict__ hdr_start, const int* __restrict__ decimals,
                                                              const int* __restrict__ values, const unsigned char* __restrict__ vlen,
                                                              const long long* __restrict__ offsets, unsigned char* __restrict__ out,
                                                              int* __restrict__ overflow, int P, int A, int M, int K, long long capacity) {
    const int r = blockIdx.y;
    const long long start = offsets[r], len = offsets[r + 1] - start;
    long long t = (long long)blockIdx.x * SDF_BLOCK + threadIdx.x;
    if (t >= len || start + t >= capacity) return;
    unsigned char* dst = out + start + t;
    bool ok;
    const int p = sdf_pose(order, r, P, &ok);
    if (t < M) {
        unsigned char ch = tmpl[t];
        const int code = map[t];
        if (code >= 0) {
            const int slot = code / 30, col = code - slot * 30, f = col / 10, c = col - f * 10;
            const int a = atom[slot];
            const bool inside = ok && a >= 0 && a < A;
            const float v = inside ? x[((long long)p * A + a) * 3 + f] : 0.f;
            const bool neg = __builtin_signbit(v);
            const double sc = fabs((double)v) * 1e4;
            bool bad = !inside || !(sc < 1e13);                          // inf / nan / absurd
            const long long m = bad ? 0 : (long long)rint(sc);
            const long long I = m / 10000;
            const int F = (int)(m - I * 10000);
            if (I >= 100000 || (neg && I >= 10000)) bad = true;
            if (bad) {
                ch = '*';
                if (c == 0) atomicAdd(overflow, 1);
            } else if (c == 5) ch = '.';
            else if (c > 5) ch = (unsigned char)('0' + (F / (int)sdf_pow10(9 - c)) % 10);
            else {
                const int q = 4 - c;                                     // this column holds the 10^q digit, q = 0 .. 4
                const int nd = sdf_digits((unsigned long long)I);
                ch = q < nd ? (unsigned char)('0' + (int)((I / (long long)sdf_pow10(q)) % 10)) : (neg && q == nd) ? '-' : ' ';
            }
        }
        *dst = ch;
        return;
    }
    t -= M;
    for (int k = 0; k < K; ++k) {
        const int h0 = hdr_start[k], hl = hdr_start[k + 1] - h0;
        const int vl = vlen[(long long)r * K + k];
        if (t < hl) { *dst = hdr[h0 + t]; return; }
        t -= hl;
        if (t < vl) { *dst = sdf_char(sdf_number(values[(long long)k * P + p], decimals[k]), (int)t); return; }
        t -= vl;
        if (t < 2) { *dst = '\n'; return; }
        t -= 2;
    }
    *dst = t < 4 ? '$' : '\n';
}

}  // namespace

PD_EXPORT int pd_sdf_format(const float* x, const unsigned char* tmpl, const int* map, const int* atom, const int* order,
                            const unsigned char* hdr, const int* hdr_start, const int* decimals, const int* values, unsigned char* vlen,
                            long long* offsets, unsigned char* out, int* overflow, int n, int P, int A, int M, int K, int fixed,
                            int longest, long long capacity, void* stream) {
    if (!x || !tmpl || !map || !atom || !offsets || !out || !overflow || n <= 0 || n > 65535 || P <= 0 || A <= 0 || M <= 0 || K < 0 ||
        K > SDF_MAX_ITEMS)
        return PD_ERR_ARG;
    if (K > 0 && (!hdr || !hdr_start || !decimals || !values || !vlen)) return PD_ERR_ARG;
    if (fixed < M + 5 + 6 * K || longest < fixed + K || capacity < (long long)n * longest) return PD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (K > 0)
        hipLaunchKernelGGL(sdf_measure_kernel, dim3((unsigned)(((long long)n * K + SDF_BLOCK - 1) / SDF_BLOCK)), dim3(SDF_BLOCK), 0, s, values,
                           decimals, order, vlen, overflow, n, P, K);
    hipLaunchKernelGGL(sdf_offsets_kernel, dim3(1), dim3(SDF_BLOCK), 0, s, vlen, offsets, (long long)fixed, n, K);
    hipLaunchKernelGGL(sdf_write_kernel, dim3((unsigned)((longest + SDF_BLOCK - 1) / SDF_BLOCK), (unsigned)n), dim3(SDF_BLOCK), 0, s, x, tmpl,
                       map, atom, order, hdr, hdr_start, decimals, values, vlen, offsets, out, overflow, P, A, M, K, capacity);
    return pd_check_launch();
}
