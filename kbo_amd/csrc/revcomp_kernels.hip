// revcomp_kernels.hip — gfx950 (MI355X, CDNA4): the reverse complement of a batch, made on the device, so that a host batch
// that is to be compared with both strands of an index crosses PCIe once (kbo_*_batch_strands) and a caller with a resident
// batch never takes it back to the host (kbo_revcomp_batch_dev / kbo_revcomp_packed_dev).
//
// Per sequence, never across a boundary: output base i = complement of input base len - 1 - i; A <-> T, C <-> G, a <-> t,
// c <-> g, every other byte as it is.
//
// Byte form: one lane per 16-byte block of the OUTPUT, aligned in memory - every store is an aligned 16-byte store, whatever
// the lengths and wherever the output begins; bytes only in the first and last block.  A block that lies inside one sequence
// (nine in ten for 150-base reads, nearly all for contigs) mirrors 16 contiguous input bytes: two aligned loads, put together
// with v_alignbyte, reversed with v_perm.  A block with a boundary in it is put together byte by byte.  The work is the same
// for millions of reads and for a handful of Mbp contigs: a workgroup covers 4 KiB of output, finds the sequences at its two
// ends once and its lanes search between them.
//
// Packed form (pack_kernels.hip has the layout): one lane per output word - the mirrored input word and its neighbour with
// their 2-bit groups reversed, shifted by the (16 - len mod 16) mod 16 padding groups, complemented (A C G T = 0 1 2 3:
// the complement is ~).
#include "device_util.hpp"

namespace kbo {
namespace {

// 0x80 in every byte of x that equals c
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x, uint32_t c)
{
    const uint32_t t = x ^ (c * 0x01010101u);
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}

// the complement of four bytes (upper and lower case alike: bit 5 is left alone)
__device__ __forceinline__ uint32_t comp4(uint32_t v)
{
    const uint32_t u = v & 0xDFDFDFDFu;
    const uint32_t at = (eq_bytes(u, 'A') | eq_bytes(u, 'T')) >> 7, cg = (eq_bytes(u, 'C') | eq_bytes(u, 'G')) >> 7;
    return v ^ (at * ('A' ^ 'T')) ^ (cg * ('C' ^ 'G'));
}

// largest s in [s0, s1) with off[s] <= p (s0 qualifies): the sequence that holds base p, empty sequences skipped
__device__ __forceinline__ uint32_t seq_of(const uint64_t *__restrict__ off, uint32_t s0, uint32_t s1, uint64_t p)
{
    while (s1 - s0 > 1) {
        const uint32_t m = s0 + (s1 - s0) / 2;
        if (off[m] <= p) s0 = m;
        else s1 = m;
    }
    return s0;
}

constexpr uint32_t kRcTile = 4096; // output bytes per workgroup: 256 lanes x 16

// out16: 16-byte aligned; base p of the reverse-complemented batch goes to out16[lead + p] (lead < 16)
__global__ __launch_bounds__(256) void revcomp_bytes_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ off, uint32_t n_seqs,
                                                            uint64_t total, uint8_t *__restrict__ out16, uint32_t lead)
{
    __shared__ uint32_t ends[2];
    const uint64_t g0 = (uint64_t)blockIdx.x * kRcTile;
    if (threadIdx.x < 2) {
        const uint64_t p_lo = g0 > lead ? g0 - lead : 0, p_hi = min(total, g0 + kRcTile - lead);
        ends[threadIdx.x] = seq_of(off, 0, n_seqs, threadIdx.x ? p_hi - 1 : p_lo);
    }
    __syncthreads();
    const uint64_t x0 = g0 + 16u * threadIdx.x;
    const uint64_t lo = max(x0, (uint64_t)lead) - lead, hi = min(x0 + 16u - lead, total); // the block's bases [lo, hi)
    if (lo >= hi) return;
    uint32_t s = seq_of(off, ends[0], ends[1] + 1u, lo);
    uint64_t b = off[s], e = off[s + 1];
    if (hi - lo == 16u && hi <= e) {
        // bases [lo, lo + 16) of sequence [b, e): the mirror of input bytes [b + e - hi, b + e - lo)
        const uint64_t src = b + e - hi;
        const uint32_t mis = (uint32_t)src & 15u;
        const uint4 *a = reinterpret_cast<const uint4 *>(in + (src - mis));
        const uint4 v0 = a[0];
        const uint4 v1 = mis ? a[1] : make_uint4(0, 0, 0, 0); // (a[1] holds bytes of the block then: below round16(total))
        const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        const uint32_t d = mis >> 2, sh = mis & 3u;
        uint32_t x[5]; // the five words the 16 bytes lie in
#pragma unroll
        for (int j = 0; j < 5; j++) x[j] = d == 0 ? w[j] : d == 1 ? w[j + 1] : d == 2 ? w[j + 2] : w[(j + 3) & 7];
        uint32_t t[4];
#pragma unroll
        for (int j = 0; j < 4; j++) t[j] = __builtin_amdgcn_alignbyte(x[j + 1], x[j], sh);
        uint4 o;
        o.x = comp4(__builtin_amdgcn_perm(0u, t[3], 0x00010203u));
        o.y = comp4(__builtin_amdgcn_perm(0u, t[2], 0x00010203u));
        o.z = comp4(__builtin_amdgcn_perm(0u, t[1], 0x00010203u));
        o.w = comp4(__builtin_amdgcn_perm(0u, t[0], 0x00010203u));
        *reinterpret_cast<uint4 *>(out16 + x0) = o;
        return;
    }
    // a boundary inside the block (or the batch's first / last block): byte by byte
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t t = 0; t < 16; t++) {
        const uint64_t g = x0 + t;
        if (g < lo + lead || g >= hi + lead) continue;
        const uint64_t p = g - lead;
        while (p >= e) { // (p < total = off[n_seqs]: s stays below n_seqs)
            s++;
            b = e;
            e = off[s + 1];
        }
        o[t >> 2] |= (uint32_t)in[b + e - 1u - p] << ((t & 3u) * 8u);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = comp4(o[j]);
    if (hi - lo == 16u) {
        *reinterpret_cast<uint4 *>(out16 + x0) = make_uint4(o[0], o[1], o[2], o[3]);
        return;
    }
#pragma unroll
    for (uint32_t t = 0; t < 16; t++)
        if (x0 + t >= lo + lead && x0 + t < hi + lead) out16[x0 + t] = (uint8_t)(o[t >> 2] >> ((t & 3u) * 8u));
}

// the 2-bit groups of a word in reverse order
__device__ __forceinline__ uint32_t rev_groups(uint32_t v)
{
    const uint32_t r = __builtin_bitreverse32(v);
    return ((r & 0xAAAAAAAAu) >> 1) | ((r & 0x55555555u) << 1);
}

__global__ __launch_bounds__(256) void revcomp_packed_kernel(const uint32_t *__restrict__ in, uint32_t n_words, const uint64_t *__restrict__ off,
                                                             uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *__restrict__ data,
                                                             const uint32_t *__restrict__ sums, uint32_t *__restrict__ out)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint32_t seq, blk;
    locate_word(w, n_seqs, uniform_wps, data, sums, seq, blk);
    const uint64_t len = off[seq + 1] - off[seq];
    const uint32_t nw = (uint32_t)((len + 15u) / 16u), w0 = w - blk;
    const uint32_t pad = (0u - (uint32_t)len) & 15u; // groups of the last input word that hold no base
    // the reversed sequence begins with those `pad` groups: output group g is reversed group g + pad
    const uint32_t a = rev_groups(in[w0 + nw - 1u - blk]);
    const uint32_t b = blk + 1u < nw ? rev_groups(in[w0 + nw - 2u - blk]) : 0u;
    uint32_t v = pad ? (a >> (2u * pad)) | (b << (32u - 2u * pad)) : a;
    v = ~v;
    if (blk + 1u == nw && pad) v &= (1u << (2u * (16u - pad))) - 1u; // padding bits of the last word: zero
    out[w] = v;
}

// the exception list mirrored within each sequence: entry x of a sequence's stretch of the list goes to the stretch's
// mirrored place, so the list ascends again
__global__ __launch_bounds__(256) void revcomp_exceptions_kernel(const uint64_t *__restrict__ pos, const uint8_t *__restrict__ byte, uint32_t n,
                                                                 uint64_t base, const uint64_t *__restrict__ off, uint32_t n_seqs, uint64_t out_base,
                                                                 uint64_t *__restrict__ pos_out, uint8_t *__restrict__ byte_out)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const uint64_t p = pos[x] - base;
    const uint32_t s = seq_of(off, 0, n_seqs, p);
    const uint64_t b = off[s], e = off[s + 1];
    uint32_t xa = 0, xb = x + 1u; // first entry at or behind b: in [0, x]
    while (xa < xb) {
        const uint32_t m = xa + (xb - xa) / 2;
        if (pos[m] - base < b) xa = m + 1u;
        else xb = m;
    }
    uint32_t ya = x, yb = n; // first entry at or behind e: in (x, n]
    while (ya < yb) {
        const uint32_t m = ya + (yb - ya) / 2;
        if (pos[m] - base < e) ya = m + 1u;
        else yb = m;
    }
    const uint32_t y = xa + ya - 1u - x;
    pos_out[y] = out_base + b + e - 1u - p;
    byte_out[y] = (uint8_t)comp4(byte[x]);
}

// ---- a slab of a host batch doubled on the device (host_batch.cpp: both strands in one launch): sequences n .. 2n-1 are the
// reverse complements of 0 .. n-1 and lie behind them
__global__ __launch_bounds__(256) void double_offsets_kernel(uint64_t *__restrict__ off, uint32_t n)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) off[n + 1u + j] = off[n] + off[j + 1u];
}

__global__ __launch_bounds__(256) void double_items_kernel(WalkItem *__restrict__ items, uint32_t n, uint64_t shift)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    WalkItem it = items[i];
    it.start += shift;
    items[n + i] = it;
}

} // namespace

hipError_t launch_revcomp_bytes(const uint8_t *d_in, const uint64_t *d_off, uint32_t n_seqs, uint64_t total, uint8_t *d_out, hipStream_t stream)
{
    if (total == 0 || n_seqs == 0) return hipSuccess;
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(d_out) & 15u);
    const uint64_t blocks = (total + lead + kRcTile - 1) / kRcTile;
    hipLaunchKernelGGL(revcomp_bytes_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, d_in, d_off, n_seqs, total, d_out - lead, lead);
    return hipGetLastError();
}

hipError_t launch_revcomp_packed(const uint32_t *d_in, uint32_t n_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps,
                                 const uint32_t *d_data, const uint32_t *d_sums, uint32_t *d_out, hipStream_t stream)
{
    if (n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(revcomp_packed_kernel, dim3((n_words + 255u) / 256u), dim3(256), 0, stream, d_in, n_words, d_off, n_seqs, uniform_wps,
                       d_data, d_sums, d_out);
    return hipGetLastError();
}

hipError_t launch_revcomp_exceptions(const uint64_t *d_pos, const uint8_t *d_byte, uint32_t n, uint64_t base, const uint64_t *d_off,
                                     uint32_t n_seqs, uint64_t out_base, uint64_t *d_pos_out, uint8_t *d_byte_out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(revcomp_exceptions_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_pos, d_byte, n, base, d_off, n_seqs,
                       out_base, d_pos_out, d_byte_out);
    return hipGetLastError();
}

hipError_t launch_double_offsets(uint64_t *d_off, uint32_t n_seqs, hipStream_t stream)
{
    if (n_seqs == 0) return hipSuccess;
    hipLaunchKernelGGL(double_offsets_kernel, dim3((n_seqs + 255u) / 256u), dim3(256), 0, stream, d_off, n_seqs);
    return hipGetLastError();
}

hipError_t launch_double_items(WalkItem *d_items, uint32_t n_items, uint64_t shift, hipStream_t stream)
{
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(double_items_kernel, dim3((n_items + 255u) / 256u), dim3(256), 0, stream, d_items, n_items, shift);
    return hipGetLastError();
}

} // namespace kbo
