// nw_band_ext.hip -- the banded extension alignment of one long pair (gsa_score_band_ext_dev,
// gsa_align_pair_band_ext_dev): the start is (0, 0), the end is the best cell of the
// diagonals lo <= j - i <= hi, the first one in row-major order.
//
// The workgroup, the strips, the lockstep super-steps and the ring are nw_band.hip's: the body is
// nw_band_dev.h's band_pair_fill in its extension mode, which adds a best value and its column per row
// of a lane, folds them per strip, and behind the last super-step reduces them over the lanes by
// shuffles and over the waves through one LDS slot per wave, with barriers only.  No wave polls
// anything and there are no atomics: every loop is bounded by T, 64, KR and the waves.
//
// The walk is band_dev::band_walk, entered through band_walk_from_start, from the cell the fill wrote
// into its result words; it is enqueued
// behind the fill and needs no host round trip.
#include "nw_band_ext.h"

#include "nw_band_dev.h"
#include "nw_lanes_trace.h"
#include "nw_strip.h"

namespace gsa {

namespace {

template <bool AFFINE, bool CODES>
__global__ __launch_bounds__(64 * kBandWaves) void nw_band_ext_kernel(const BandDesc* descs, const int* subst, int ssz, int go,
                                                                       int ge)
{
    __shared__ int tab[32 * 32];
    __shared__ int2 ring[kBandWaves][band_dev::RQ][64];
    __shared__ int4 best[kBandWaves];
    band_dev::band_load_tab<CODES>(tab, subst, ssz);
    __syncthreads();
    const BandDesc d = descs[blockIdx.x];
    band_dev::band_pair_fill<AFFINE, CODES, true>(d, tab, &ring[0][0][0], ssz, go, ge, best);
}

// One lane (band_dev::band_walk), from the end cell in a.start.
__global__ __launch_bounds__(64) void nw_band_ext_walk_kernel(BandWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    band_dev::band_walk_from_start(a);
}

template <bool AFFINE, bool CODES>
hipError_t launch_fill(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                       hipStream_t st)
{
    auto kern = nw_band_ext_kernel<AFFINE, CODES>;
    hipError_t e = record_foot((const void*)kern, 0, 64 * waves, npairs);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(npairs), dim3(64 * waves), 0, st, descs, subst, substsz, go, ge);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_band_ext(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                           bool codes, const BandWalkArgs* w, hipEvent_t* ev, hipStream_t st)
{
    if (npairs < 1 || waves < 1 || waves > kBandWaves || (w && !w->start)) return hipErrorInvalidValue;
    const bool affine = go != ge;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e = codes ? (affine ? launch_fill<true, true>(descs, npairs, waves, subst, substsz, go, ge, st)
                                   : launch_fill<false, true>(descs, npairs, waves, subst, substsz, go, ge, st))
                         : (affine ? launch_fill<true, false>(descs, npairs, waves, subst, substsz, go, ge, st)
                                   : launch_fill<false, false>(descs, npairs, waves, subst, substsz, go, ge, st));
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    if (w)
    {
        hipLaunchKernelGGL(nw_band_ext_walk_kernel, dim3(1), dim3(64), 0, st, *w);
        e = hipGetLastError();
    }
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
