// refset_walk.hpp — one lane's chunk of the reference-set walks, for refset_kernels.hip (the form in LDS) and refset_wide_kernels.hip
// (the form in global memory): k - 1 warm-up bases for the state, then a depth per base; the query is read 16 bytes at a time and the
// depths are stored 16 at a time.  The step is refset_step.hpp's, over the kernel's accessor.  Device code only.
#pragma once
#include "device_util.hpp"
#include "refset_step.hpp"

namespace kbo {

// refset_step.hpp's accessor over a packed form (kernels.hpp "LDS form") of n rows at `form`, in LDS or in global memory: a rank is
// one 8-byte load (the compiler knows the address space of a staged form once the kernel is inlined: ds_read_b64 there)
struct PackedForm {
    const uint2 *rank_;
    const uint8_t *lcs_;
    __device__ __forceinline__ PackedForm(const uint4 *form, uint32_t n)
        : rank_(reinterpret_cast<const uint2 *>(form)), lcs_(reinterpret_cast<const uint8_t *>(form + refset_rank_units(n)))
    {
    }
    __device__ __forceinline__ refstep::Entry rank(uint32_t block, uint32_t c) const
    {
        const uint2 e = rank_[block * 4u + c];
        return refstep::Entry{e.x, e.y};
    }
    __device__ __forceinline__ uint32_t lcs(uint32_t i) const { return lcs_[i]; }
};

// item: { first base in q, first byte in ms, bases | warm-up bases << 16, 0 } (kernels.hpp RefsetWalkArgs); n: rows of the form
template <typename Acc>
__device__ __forceinline__ void refset_walk_chunk(const Acc &x, uint32_t n, uint32_t k, const uint4 &item, const uint8_t *q_base, uint8_t *ms_base)
{
    const uint32_t len = item.z & 0xFFFFu, warm = item.z >> 16;
    const uint8_t *q = q_base + item.x;
    uint32_t l = 0, r = n, d = 0;
    for (uint32_t p = 0; p < warm; p += 16u) { // k - 1 bases in front of the chunk: state only
        const uint4 v = ld16u(q, p);
        uint64_t lo = (uint64_t)v.x | (uint64_t)v.y << 32, hi = (uint64_t)v.z | (uint64_t)v.w << 32;
        const uint32_t nb = min(16u, warm - p);
        for (uint32_t j = 0; j < nb; j++) {
            refstep::step(x, n, k, (uint32_t)lo & 0xFFu, l, r, d);
            lo = lo >> 8 | hi << 56;
            hi >>= 8;
        }
    }
    uint8_t *out = ms_base + item.y;
    for (uint32_t p = warm; p < len; p += 16u) {
        const uint4 v = ld16u(q, p);
        uint64_t lo = (uint64_t)v.x | (uint64_t)v.y << 32, hi = (uint64_t)v.z | (uint64_t)v.w << 32;
        uint64_t olo = 0, ohi = 0; // the depths enter at the top byte and move down
        const uint32_t nb = min(16u, len - p);
        for (uint32_t j = 0; j < nb; j++) {
            refstep::step(x, n, k, (uint32_t)lo & 0xFFu, l, r, d);
            lo = lo >> 8 | hi << 56;
            hi >>= 8;
            olo = olo >> 8 | ohi << 56;
            ohi = ohi >> 8 | (uint64_t)d << 56;
        }
        for (uint32_t j = nb; j < 16u; j++) {
            olo = olo >> 8 | ohi << 56;
            ohi >>= 8;
        }
        const uint4 o = make_uint4((uint32_t)olo, (uint32_t)(olo >> 32), (uint32_t)ohi, (uint32_t)(ohi >> 32));
        if (nb == 16u) st16u(out, p - warm, o);
        else st_partial(out + (p - warm), o, nb);
    }
}

} // namespace kbo
