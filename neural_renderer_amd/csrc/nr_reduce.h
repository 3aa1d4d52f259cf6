// nr_reduce.h -- fixed-order sums and scans (DESIGN "Fixed-order sums and scans"): the one definition of the orders behind "no
// atomics: the same bits in every run, and an image alone gives the bits it has inside a batch".  nr_device.h includes it.
//
// A SUM over an image, in double, takes three steps, each in one fixed order:
//   wave_sum      the wave's xor butterfly, v = v + v[lane ^ o] for o = 32, 16, .., 1: every lane ends with the same bits;
//   waves_sum     the waves' sums from LDS in wave order, starting FROM WAVE 0's VALUE (not from 0.0: -0.0 stays -0.0);
//                 block_sums is the two together for the N sums of a workgroup;
//   ordered_sum   the workgroups' partials of an image in block order, starting from 0.0, by one thread.
// What a thread adds up before the butterfly, and in which order, is the kernel's own and stated at its head.
//
// A SCAN over the threads of a workgroup is a wave's inclusive scan (wave_incl_scan through shuffles for any element type,
// wave_incl_scan_dpp for ints without the LDS crossbar), then block_excl_scan over the waves.  Integers: the order cannot
// change the bits, the helpers are here to exist once.
#pragma once
#include "nr_device.h"

namespace nr {

// the sum of v over the 64 lanes, in every lane (float or double)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// the waves' sums ws[0 .. NW) in wave order from wave 0's value
template <int NW>
__device__ __forceinline__ double waves_sum(const double (&ws)[NW])
{
    double s = ws[0];
#pragma unroll
    for (int w = 1; w < NW; w++) s += ws[w];
    return s;
}

// The sums of v[0 .. n) over a workgroup of NT threads: thread k < n returns sum k, the others 0.  Every thread of the workgroup
// must call it, with the same n; it holds one barrier, so a second call (of the same NT and N) needs a barrier in front.
template <int NT, int N>
__device__ __forceinline__ double block_sums(const double (&v)[N], int n)
{
    __shared__ double ws[N][NT / WAVE];
#pragma unroll
    for (int k = 0; k < N; k++) {
        if (k < n) {
            const double x = wave_sum(v[k]);
            if ((threadIdx.x & (WAVE - 1)) == 0) ws[k][threadIdx.x / WAVE] = x;
        }
    }
    __syncthreads();
    return (int)threadIdx.x < n ? waves_sum(ws[threadIdx.x]) : 0.0;
}

// one sum: valid in thread 0
template <int NT>
__device__ __forceinline__ double block_sum(double v)
{
    const double one[1] = {v};
    return block_sums<NT>(one, 1);
}

// p[0] + p[stride] + .. (n terms, n may be 0) added to 0.0 in index order: the partials of an image in block order
__device__ __forceinline__ double ordered_sum(const double *__restrict__ p, int n, size_t stride)
{
    double s = 0.0;
    for (int i = 0; i < n; i++) s += p[(size_t)i * stride];
    return s;
}

// inclusive prefix sum over the 64 lanes of a wave (lane = threadIdx.x & 63): lane l returns v of the lanes 0 .. l
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane)
{
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const T t = __shfl_up(v, o, WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

// inclusive prefix sum over the 64 lanes with DPP moves only (no LDS crossbar round trips): Hillis-Steele inside each row of 16
// lanes, then the row totals are passed on (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3)
__device__ __forceinline__ int wave_incl_scan_dpp(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
}

// Exclusive scan of one value per thread over the workgroup of NT threads, given `inc`, the wave's inclusive scan of v (by
// either scan above, or several of them on the fields of a packed word).  Returns the exclusive prefix, *total = the sum.
// s_tmp: NT / 64 words of LDS, free again on return (two barriers); every thread of the workgroup must call it.
template <int NT, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T inc, T *s_tmp, T *total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 63) s_tmp[wave] = inc;
    __syncthreads();
    T woff = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) {
        const T c = s_tmp[w];
        if (w < wave) woff += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return woff + inc - v;
}

}  // namespace nr
