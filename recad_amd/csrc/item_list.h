// The neighbour-list machinery of the item-item fits (itemknn.hip, rp3beta.hip): one 256-thread workgroup per item keeps a
// running list of the largest 64-bit keys (bits of w) << 32 | (0xFFFFFFFF - j) -- all distinct, descending key = (w descending,
// j ascending) -- merged across bands of candidates through a pending area and a bitonic sort.  Beside it what the item-item
// files share: the band refusal and automatic band, the score term, and the row length from which a band segment is searched
// (ease.hip's Gram kernel walks by it too).
#pragma once
#include "common.h"

typedef unsigned long long ik_key;

static constexpr int kIkThreads = 256;
static constexpr int kIkKeys = 512;                             // ik_key buf[512]: [0, 128) running list | [128, 384) pending | [384, 512) zeros
static constexpr int kIkPending = 256;                          // one chunk of candidates (one per thread) always fits an empty pending area
static constexpr int kIkMiscBytes = 64;
// LDS of one neighbour workgroup: ik_key buf[kIkKeys] | uint32 misc[16] | the accumulators of one band; every offset a multiple of 16
static constexpr int kIkNbrScratchBytes = 8 * kIkKeys + kIkMiscBytes;
static_assert(RK_KNN_MAX_K == 128 && kIkPending == kIkThreads, "the list layout is written for 128 slots");
// a row longer than this is binary-searched for the band's segment; a shorter one is strided whole and filtered (two dependent
// searches cost more than two strides of the row)
static constexpr int kIkSearchFrom = 128;

// the automatic band (band == 0: the catalogue in equal bands of at most auto_band, rounded up to 64) or the refusal of a bad one
static inline int ik_resolve_band(const char *who, int *band, int max_band, int auto_band, int n_items)
{
    if (*band != 0 && (*band < 64 || *band > max_band || *band % 64))
        RK_FAIL(RK_EINVAL, "%s: band = %d (0, or a multiple of 64 in 64..%d)", who, *band, max_band);
    if (*band == 0) {
        const int n_bands = (n_items + auto_band - 1) / auto_band;
        *band = (((n_items + n_bands - 1) / n_bands) + 63) / 64 * 64;
    }
    return RK_OK;
}

// s + fl(w * q): two roundings, never one fused multiply-add
__device__ __forceinline__ float ik_add_term(float s, float w, float q)
{
#pragma clang fp contract(off)
    const float term = w * q;
    return s + term;
}

// How many threads of the block pass `pred`; every thread gets the count.  One barrier: the four per-wave counts alternate
// between two sets of slots, so a wave that runs ahead into the next call writes the other set.  (__syncthreads_count would
// bring a static LDS variable, and the largest band leaves no room for one.)
__device__ __forceinline__ int ik_block_count(bool pred, unsigned *slots, int &phase)
{
    const unsigned long long m = __ballot(pred);
    unsigned *s = slots + 4 * (phase & 1);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    phase ^= 1;
    return (int)((s[0] + s[1]) + (s[2] + s[3]));
}

// descending bitonic sort of buf[0, 512), one compare-exchange per thread and step.  All threads of the block call it; it
// begins and ends with a barrier.
static __device__ void ik_sort(ik_key *buf)
{
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll 1
    for (int size = 2; size <= kIkKeys; size <<= 1) {
#pragma unroll 1
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int pos = (tid / stride) * 2 * stride + (tid % stride), j = pos + stride;
            const ik_key a = buf[pos], b = buf[j];
            const bool desc = (pos & size) == 0;
            if ((a < b) == desc && a != b) { buf[pos] = b; buf[j] = a; }
            __syncthreads();
        }
    }
}
