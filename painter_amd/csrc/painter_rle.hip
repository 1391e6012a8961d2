// COCO run-length encoding of bit masks, and back (include/painter_rle.h; tests/painter_rle_host.py is the definition).
//
// Encode, six launches, no pool of runs:
//   rle_cols_kernel      one thread per (mask, column): walks the column's h bits, counts transitions (the top pixel compares with the
//                        bottom of the previous column), set pixels, the row extent, and keeps the column's last three transitions
//   rle_scan_cols_kernel one workgroup per mask: exclusive scans over the columns, in chunks of 256 with a carry -- the column's base in
//                        the mask's runs, and the three transitions BEFORE the column (operator: append and keep the last three);
//                        area and box
//   rle_chars_kernel<0>  the column walk again: count i with the transitions p_i .. p_(i-3) at hand is
//                        x = (p_i - p_(i-1)) - (p_(i-2) - p_(i-3)); the walk counts x's characters
//   rle_scan_chars_kernel one workgroup per mask: the column's base in the mask's string
//   rle_scan_masks_kernel one workgroup: each mask's base in the pool, header, overflow
//   rle_chars_kernel<1>  the walk a third time, writing the characters -- unless the header says they do not fit
// Decode: rle_parse_kernel, one workgroup per mask (characters -> values by a scan over the value ends; the two delta chains and the
// positions by scans in the same chunk loop); rle_fill_kernel, one thread per (mask, column): binary search of the column's first run,
// integer atomicOr per set pixel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/painter_rle.h"
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_SLOTS = 65535;
constexpr int64_t MAX_ELEMS = (int64_t)1 << 27;          // input elements of one mask in the decode (int64 sums stay exact)

bool shape_ok(int h, int w, int n) { return h >= 1 && w >= 1 && n >= 1 && n <= MAX_SLOTS && (int64_t)h * w < ((int64_t)1 << 31); }

struct EncLayout { int64_t A, B, col_base, col_chars, col_char_base, mask_runs, mask_chars, mask_char_base, total; };
EncLayout enc_layout(int w, int n) {
    EncLayout L;
    const int64_t c = (int64_t)n * w;
    int64_t o = 0;
    L.A = o; o = up16(o + 16 * c);
    L.B = o; o = up16(o + 16 * c);
    L.col_char_base = o; o = up16(o + 8 * c);
    L.col_base = o; o = up16(o + 4 * c);
    L.col_chars = o; o = up16(o + 4 * c);
    L.mask_chars = o; o = up16(o + 8 * (int64_t)n);
    L.mask_char_base = o; o = up16(o + 8 * (int64_t)n);
    L.mask_runs = o; o = up16(o + 4 * (int64_t)n);
    L.total = o;
    return L;
}

// ---- scans of a 256-thread workgroup.  op(earlier, later); lds: TPB elements.  -> inclusive value; lds[t] holds it for every t after the
// call, and the caller synchronises before lds is written again.
template <typename T, typename Op>
DEVI T block_scan(T v, T* lds, Op op) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {
        T o = v;
        if (t >= d) o = op(lds[t - d], v);
        __syncthreads();
        v = o;
        lds[t] = v;
        __syncthreads();
    }
    return v;
}

struct AddU32 { DEVI uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct AddU64 { DEVI u64 operator()(u64 a, u64 b) const { return a + b; } };
struct AddI64 { DEVI int64_t operator()(int64_t a, int64_t b) const { return a + b; } };
struct Pair { int64_t odd, even; };
struct AddPair { DEVI Pair operator()(Pair a, Pair b) const { return Pair{a.odd + b.odd, a.even + b.even}; } };
// x = how many of y, z, w hold a transition (0 .. 3); y the latest, z the one before it, w the one before that
struct Last3 { DEVI uint4 operator()(uint4 a, uint4 b) const {
    if (b.x == 0) return a;
    if (b.x >= 3) return b;
    const uint32_t n = min(3u, a.x + b.x);
    return b.x == 1 ? make_uint4(n, b.y, a.y, a.z) : make_uint4(n, b.y, b.z, a.y);
} };

DEVI uint32_t bit_at(const uint32_t* __restrict__ m, uint32_t p) { return (m[p >> 5] >> (p & 31)) & 1u; }
DEVI int clamped_count(const int* count, int n_cap) { return clampi(count[0], 0, n_cap); }

// ---- encode
__global__ __launch_bounds__(64) void rle_cols_kernel(const uint32_t* __restrict__ masks, const int* __restrict__ count, uint4* __restrict__ A,
                                                     uint4* __restrict__ B, int h, int w, int words, int n_cap) {
    const int m = blockIdx.y;
    const int64_t x64 = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (m >= clamped_count(count, n_cap) || x64 >= w) return;
    const uint32_t x = (uint32_t)x64;
    const uint32_t* bits = masks + (size_t)m * words;
    uint32_t prev = x ? bit_at(bits, (uint32_t)(h - 1) * w + x - 1) : 0u;
    uint32_t trans = 0, nset = 0, ymin = 0xffffffffu, ymax = 0, q1 = 0, q2 = 0, q3 = 0;
    uint32_t p = x, j = x * (uint32_t)h;                    // p = y * w + x, j = x * h + y: both < h * w < 2^31
    for (int y = 0; y < h; ++y, p += w, ++j) {
        const uint32_t v = bit_at(bits, p);
        if (v != prev) { ++trans; q3 = q2; q2 = q1; q1 = j; prev = v; }
        if (v) { ++nset; ymin = min(ymin, (uint32_t)y); ymax = (uint32_t)y; }
    }
    const size_t at = (size_t)m * w + x;
    A[at] = make_uint4(trans, nset, ymin, ymax);
    B[at] = make_uint4(min(trans, 3u), q1, q2, q3);
}

__global__ __launch_bounds__(TPB) void rle_scan_cols_kernel(const int* __restrict__ count, const uint4* __restrict__ A, uint4* __restrict__ B,
                                                           uint32_t* __restrict__ col_base, uint32_t* __restrict__ mask_runs,
                                                           pa_rle_record* __restrict__ records, int w, int n_cap) {
    __shared__ uint32_t s_u32[TPB];
    __shared__ uint4 s_l3[TPB];
    __shared__ uint32_t s_area, s_xs, s_ys, s_xe, s_ye;
    const int m = blockIdx.x, t = threadIdx.x;
    if (m >= clamped_count(count, n_cap)) return;                       // uniform
    if (t == 0) { s_area = 0; s_xs = 0xffffffffu; s_ys = 0xffffffffu; s_xe = 0; s_ye = 0; }
    uint32_t carry = 0, area = 0, xs = 0xffffffffu, ys = 0xffffffffu, xe = 0, ye = 0;
    uint4 carry3 = make_uint4(0, 0, 0, 0);
    for (int64_t base = 0; base < w; base += TPB) {
        const int64_t x = base + t;
        const bool in = x < w;
        const size_t at = (size_t)m * w + (size_t)x;
        const uint4 a = in ? A[at] : make_uint4(0, 0, 0, 0);
        const uint4 b = in ? B[at] : make_uint4(0, 0, 0, 0);
        const uint32_t incl = block_scan(a.x, s_u32, AddU32());
        const uint32_t total = s_u32[TPB - 1];
        block_scan(b, s_l3, Last3());
        const uint4 before = t ? s_l3[t - 1] : make_uint4(0, 0, 0, 0);
        const uint4 total3 = s_l3[TPB - 1];
        __syncthreads();
        if (in) {
            col_base[at] = carry + incl - a.x;
            B[at] = Last3()(carry3, before);
            if (a.y) { area += a.y; xs = min(xs, (uint32_t)x); xe = max(xe, (uint32_t)x); ys = min(ys, a.z); ye = max(ye, a.w); }
        }
        carry += total;
        carry3 = Last3()(carry3, total3);
    }
    if (area) { atomicAdd(&s_area, area); atomicMin(&s_xs, xs); atomicMin(&s_ys, ys); atomicMax(&s_xe, xe); atomicMax(&s_ye, ye); }
    __syncthreads();
    if (t == 0) {
        pa_rle_record* r = records + m;
        r->runs = carry + 1;
        r->area = s_area;
        const bool any = s_area != 0;
        r->bbox[0] = any ? (int)s_xs : 0;
        r->bbox[1] = any ? (int)s_ys : 0;
        r->bbox[2] = any ? (int)(s_xe - s_xs + 1) : 0;
        r->bbox[3] = any ? (int)(s_ye - s_ys + 1) : 0;
        mask_runs[m] = carry + 1;
    }
}

// rleToString's groups of count i that ends at transition p (or at h * w); WRITE: emitted at out.  -> their number, 1 .. 7
template <bool WRITE>
DEVI uint32_t emit_count(uint32_t i, uint32_t p, uint32_t q1, uint32_t q2, uint32_t q3, uint8_t* out) {
    int32_t x = (int32_t)(p - (i >= 1 ? q1 : 0u));
    if (i >= 3) x -= (int32_t)(q2 - q3);
    uint32_t n = 0;
    bool more;
    do {
        int32_t c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        if (WRITE) out[n] = (uint8_t)(c + 48);
        ++n;
    } while (more);
    return n;
}

template <bool WRITE>
__global__ __launch_bounds__(64) void rle_chars_kernel(const uint32_t* __restrict__ masks, const int* __restrict__ count,
                                                      const uint4* __restrict__ B, const uint32_t* __restrict__ col_base,
                                                      uint32_t* __restrict__ col_chars, const u64* __restrict__ col_char_base,
                                                      const u64* __restrict__ mask_char_base, const pa_rle_header* __restrict__ header,
                                                      uint8_t* __restrict__ pool, int h, int w, int words, int n_cap) {
    const int m = blockIdx.y;
    const int64_t x64 = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (m >= clamped_count(count, n_cap) || x64 >= w) return;
    if (WRITE && header->overflow) return;
    const uint32_t x = (uint32_t)x64;
    const uint32_t* bits = masks + (size_t)m * words;
    const size_t at = (size_t)m * w + x;
    const uint4 b = B[at];
    uint32_t i = col_base[at], q1 = b.y, q2 = b.z, q3 = b.w;
    uint8_t* out = WRITE ? pool + mask_char_base[m] + col_char_base[at] : nullptr;
    uint32_t prev = x ? bit_at(bits, (uint32_t)(h - 1) * w + x - 1) : 0u;
    uint32_t chars = 0;
    uint32_t p = x, j = x * (uint32_t)h;
    for (int y = 0; y < h; ++y, p += w, ++j) {
        const uint32_t v = bit_at(bits, p);
        if (v != prev) {
            chars += emit_count<WRITE>(i, j, q1, q2, q3, out + chars);
            ++i; q3 = q2; q2 = q1; q1 = j; prev = v;
        }
    }
    if (x == (uint32_t)(w - 1)) chars += emit_count<WRITE>(i, (uint32_t)h * (uint32_t)w, q1, q2, q3, out + chars);      // the last run ends at h * w
    if (!WRITE) col_chars[at] = chars;
}

__global__ __launch_bounds__(TPB) void rle_scan_chars_kernel(const int* __restrict__ count, const uint32_t* __restrict__ col_chars,
                                                            u64* __restrict__ col_char_base, u64* __restrict__ mask_chars, int w, int n_cap) {
    __shared__ u64 s[TPB];
    const int m = blockIdx.x, t = threadIdx.x;
    if (m >= clamped_count(count, n_cap)) return;
    u64 carry = 0;
    for (int64_t base = 0; base < w; base += TPB) {
        const int64_t x = base + t;
        const size_t at = (size_t)m * w + (size_t)x;
        const u64 v = x < w ? col_chars[at] : 0;
        const u64 incl = block_scan(v, s, AddU64());
        const u64 total = s[TPB - 1];
        __syncthreads();
        if (x < w) col_char_base[at] = carry + incl - v;
        carry += total;
    }
    if (t == 0) mask_chars[m] = carry;
}

__global__ __launch_bounds__(TPB) void rle_scan_masks_kernel(const int* __restrict__ count, const uint32_t* __restrict__ mask_runs,
                                                            const u64* __restrict__ mask_chars, u64* __restrict__ mask_char_base,
                                                            pa_rle_record* __restrict__ records, pa_rle_header* __restrict__ header,
                                                            int64_t char_cap, int n_cap) {
    __shared__ u64 s[TPB];
    const int t = threadIdx.x, n = clamped_count(count, n_cap);
    u64 carry = 0, runs = 0;
    for (int base = 0; base < n; base += TPB) {
        const int m = base + t;
        const u64 v = m < n ? mask_chars[m] : 0;
        const u64 incl = block_scan(v, s, AddU64());
        const u64 total = s[TPB - 1];
        __syncthreads();
        const u64 r = block_scan((u64)(m < n ? mask_runs[m] : 0), s, AddU64());
        (void)r;
        runs += s[TPB - 1];
        __syncthreads();
        if (m < n) {
            mask_char_base[m] = carry + incl - v;
            records[m].char_offset = (int64_t)(carry + incl - v);
            records[m].char_count = (int64_t)v;
        }
        carry += total;
    }
    if (t == 0) {
        header->runs = (int64_t)runs;
        header->chars = (int64_t)carry;
        header->overflow = (int64_t)carry > char_cap ? 1 : 0;
        header->count = n;
    }
}

// ---- decode
DEVI int first_flag(uint32_t bits) {
    return bits & (1u << 7) ? 7 : bits & (1u << 4) ? 4 : bits & (1u << 3) ? 3 : bits & (1u << 2) ? 2 : bits & (1u << 1) ? 1 : 0;
}

__global__ __launch_bounds__(TPB) void rle_parse_kernel(const void* __restrict__ pool, int compressed, const int64_t* __restrict__ spans,
                                                       int64_t pool_len, int64_t run_cap, int64_t npix, int64_t* __restrict__ vals,
                                                       int* __restrict__ n_runs, int* __restrict__ flags) {
    __shared__ int64_t s_i64[TPB];
    __shared__ Pair s_pair[TPB];
    __shared__ uint32_t s_bits;
    const int m = blockIdx.x, t = threadIdx.x;
    const int64_t off = spans[2 * m], len = spans[2 * m + 1];
    if (off < 0 || len < 0 || off > pool_len || len > pool_len - off || off + len > run_cap || len >= MAX_ELEMS) {       // uniform
        if (t == 0) {
            flags[m] = (off < 0 || len < 0 || off > pool_len || len > pool_len - off) ? 6 : 5;
            n_runs[m] = 0;
        }
        return;
    }
    if (t == 0) s_bits = 0;
    __syncthreads();
    int64_t* v = vals + off;
    const int n_in = (int)len;
    int n_vals = n_in;
    if (compressed) {
        const uint8_t* s = (const uint8_t*)pool + off;
        int carry = 0;
        for (int base = 0; base < n_in; base += TPB) {
            const int idx = base + t;
            const int c = idx < n_in ? (int)s[idx] - 48 : 0x20;
            if (idx < n_in && (unsigned)c > 63u) atomicOr(&s_bits, 1u << 7);
            const bool end = idx < n_in && !(c & 0x20);
            const int64_t incl = block_scan((int64_t)end, s_i64, AddI64());
            const int total = (int)s_i64[TPB - 1];
            __syncthreads();
            if (end) {
                int g = 1, j = idx - 1;
                while (j >= 0 && g <= 7 && (((int)s[j] - 48) & 0x20)) { ++g; --j; }
                if (g > 7) atomicOr(&s_bits, 1u << 4);
                else {
                    int64_t x = 0;
                    for (int q = 0; q < g; ++q) x |= (int64_t)(((int)s[j + 1 + q] - 48) & 0x1f) << (5 * q);
                    if (c & 0x10) x |= -((int64_t)1 << (5 * g));
                    v[carry + (int)incl - 1] = x;
                }
            }
            carry += total;
        }
        n_vals = carry;
        if (t == 0 && n_in > 0 && (((int)s[n_in - 1] - 48) & 0x20)) atomicOr(&s_bits, 1u << 3);
    }
    __syncthreads();
    if (s_bits & ~6u) {                                                   // uniform: 7, 4 or 3 -- the values are not all there
        if (t == 0) { flags[m] = first_flag(s_bits); n_runs[m] = 0; }
        return;
    }
    const uint32_t* u = (const uint32_t*)pool + off;
    int64_t carry_odd = 0, carry_even = 0, carry_pos = 0;
    for (int base = 0; base < n_vals; base += TPB) {
        const int i = base + t;
        const bool in = i < n_vals;
        int64_t cnt = 0;
        if (compressed) {
            const int64_t x = in ? v[i] : 0;
            const Pair mine = Pair{(in && (i & 1)) ? x : 0, (in && i > 0 && !(i & 1)) ? x : 0};
            const Pair incl = block_scan(mine, s_pair, AddPair());
            const Pair total = s_pair[TPB - 1];
            __syncthreads();
            cnt = i == 0 ? x : (i & 1) ? carry_odd + incl.odd : carry_even + incl.even;
            carry_odd += total.odd;
            carry_even += total.even;
        } else if (in) {
            cnt = (int64_t)u[i];
        }
        if (in && cnt < 0) atomicOr(&s_bits, 1u << 2);
        cnt = !in ? 0 : cnt < 0 ? 0 : cnt > npix ? npix + 1 : cnt;      // a count beyond h * w: the sum is wrong whatever follows
        const int64_t pos = block_scan(cnt, s_i64, AddI64());
        const int64_t total = s_i64[TPB - 1];
        __syncthreads();
        if (in) v[i] = carry_pos + pos;
        carry_pos += total;
    }
    if (t == 0 && carry_pos != npix) atomicOr(&s_bits, 1u << 1);
    __syncthreads();
    if (t == 0) {
        const int f = first_flag(s_bits);
        flags[m] = f;
        n_runs[m] = f ? 0 : n_vals;
    }
}

__global__ __launch_bounds__(64) void rle_fill_kernel(const int64_t* __restrict__ spans, const int64_t* __restrict__ vals,
                                                     const int* __restrict__ n_runs, const int* __restrict__ flags, uint32_t* __restrict__ out,
                                                     int h, int w, int words) {
    const int m = blockIdx.y;
    const int64_t x64 = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int nr = n_runs[m];
    if (x64 >= w || flags[m] != 0 || nr < 1) return;
    const uint32_t x = (uint32_t)x64;
    const int64_t* E = vals + spans[2 * m];                   // E[r] = where run r ends; E[nr - 1] = h * w
    const int64_t j0 = (int64_t)x * h, j1 = j0 + h;
    int lo = 0, hi = nr - 1;                                   // the first run that ends after j0
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (E[mid] > j0) hi = mid; else lo = mid + 1;
    }
    uint32_t* bits = out + (size_t)m * words;
    int64_t start = j0;
    for (int r = lo; r < nr && start < j1; ++r) {
        const int64_t e = min(E[r], j1);
        if (r & 1)
            for (int64_t j = start; j < e; ++j) {
                const uint32_t p = (uint32_t)(j - j0) * (uint32_t)w + x;
                atomicOr(&bits[p >> 5], 1u << (p & 31));
            }
        start = max(start, e);
    }
}

}  // namespace

extern "C" {

int64_t pa_rle_encode_workspace_bytes(int h, int w, int n_cap) {
    if (!shape_ok(h, w, n_cap)) return -1;
    return enc_layout(w, n_cap).total;
}

int pa_rle_encode(const void* masks_u32, const void* count, int h, int w, int n_cap, void* workspace, int64_t char_cap, void* out_header,
                  void* out_records, void* out_pool, hipStream_t stream) {
    if (!masks_u32 || !count || !workspace || !out_header || !out_records || !out_pool || !shape_ok(h, w, n_cap) || char_cap < 0 ||
        ((uintptr_t)workspace & 15) || ((uintptr_t)out_header & 7) || ((uintptr_t)out_records & 7) || ((uintptr_t)masks_u32 & 3) ||
        ((uintptr_t)count & 3))
        return (int)hipErrorInvalidValue;
    const EncLayout L = enc_layout(w, n_cap);
    char* ws = (char*)workspace;
    const uint32_t* masks = (const uint32_t*)masks_u32;
    const int* cnt = (const int*)count;
    uint4* A = (uint4*)(ws + L.A);
    uint4* B = (uint4*)(ws + L.B);
    uint32_t* col_base = (uint32_t*)(ws + L.col_base);
    uint32_t* col_chars = (uint32_t*)(ws + L.col_chars);
    u64* col_char_base = (u64*)(ws + L.col_char_base);
    uint32_t* mask_runs = (uint32_t*)(ws + L.mask_runs);
    u64* mask_chars = (u64*)(ws + L.mask_chars);
    u64* mask_char_base = (u64*)(ws + L.mask_char_base);
    pa_rle_record* records = (pa_rle_record*)out_records;
    pa_rle_header* header = (pa_rle_header*)out_header;
    const int words = (int)(((int64_t)h * w + 31) / 32);
    const dim3 cols((unsigned)((w + 63) / 64), (unsigned)n_cap);
    PA_LAUNCH_TRY(rle_cols_kernel, cols, dim3(64), 0, stream, masks, cnt, A, B, h, w, words, n_cap);
    PA_LAUNCH_TRY(rle_scan_cols_kernel, dim3((unsigned)n_cap), dim3(TPB), 0, stream, cnt, A, B, col_base, mask_runs, records, w, n_cap);
    PA_LAUNCH_TRY(rle_chars_kernel<false>, cols, dim3(64), 0, stream, masks, cnt, B, col_base, col_chars, col_char_base, mask_char_base, header,
                  (uint8_t*)out_pool, h, w, words, n_cap);
    PA_LAUNCH_TRY(rle_scan_chars_kernel, dim3((unsigned)n_cap), dim3(TPB), 0, stream, cnt, col_chars, col_char_base, mask_chars, w, n_cap);
    PA_LAUNCH_TRY(rle_scan_masks_kernel, dim3(1), dim3(TPB), 0, stream, cnt, mask_runs, mask_chars, mask_char_base, records, header, char_cap,
                  n_cap);
    PA_LAUNCH(rle_chars_kernel<true>, cols, dim3(64), 0, stream, masks, cnt, B, col_base, col_chars, col_char_base, mask_char_base, header,
              (uint8_t*)out_pool, h, w, words, n_cap);
    LAUNCH_CHECK();
}

int64_t pa_rle_decode_workspace_bytes(int n, int h, int w, int64_t run_cap) {
    if (!shape_ok(h, w, n) || run_cap < 0 || run_cap > ((int64_t)1 << 56)) return -1;
    return up16(8 * run_cap) + up16(4 * (int64_t)n);
}

int pa_rle_decode(const void* pool, int compressed, const void* spans, int n, int h, int w, int64_t pool_len, int64_t run_cap,
                  void* workspace, void* out_bits, void* out_flags, hipStream_t stream) {
    if (!pool || !spans || !workspace || !out_bits || !out_flags || !shape_ok(h, w, n) || pool_len < 0 || run_cap < 0 ||
        run_cap > ((int64_t)1 << 56) || ((uintptr_t)workspace & 15) || ((uintptr_t)spans & 7) || ((uintptr_t)out_bits & 3) ||
        ((uintptr_t)out_flags & 3) || (!compressed && ((uintptr_t)pool & 3)))
        return (int)hipErrorInvalidValue;
    const int64_t npix = (int64_t)h * w;
    const int words = (int)((npix + 31) / 32);
    int64_t* vals = (int64_t*)workspace;
    int* n_runs = (int*)((char*)workspace + up16(8 * run_cap));
    PA_TRY(hipMemsetAsync(out_bits, 0, 4 * (size_t)n * words, stream));
    PA_LAUNCH_TRY(rle_parse_kernel, dim3((unsigned)n), dim3(TPB), 0, stream, pool, compressed, (const int64_t*)spans, pool_len, run_cap, npix,
                  vals, n_runs, (int*)out_flags);
    PA_LAUNCH(rle_fill_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)n), dim3(64), 0, stream, (const int64_t*)spans, (const int64_t*)vals,
              (const int*)n_runs, (const int*)out_flags, (uint32_t*)out_bits, h, w, words);
    LAUNCH_CHECK();
}

}  // extern "C"
