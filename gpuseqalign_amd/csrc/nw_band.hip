// nw_band.hip -- the banded alignment of one long pair (gsa_score_band_dev, gsa_align_pair_band_dev;
// DESIGN.md 2.2p): global alignment with linear or affine gaps inside the diagonals lo <= j - i <= hi.
//
// One workgroup of up to 16 waves takes a pair.  Strip s (rows s TR + 1 ... (s + 1) TR) runs on wave
// s mod NWV; lane l holds KR = 4 rows and runs one column behind lane l - 1, whose last row it takes
// with a wave-wide shift by one lane (DPP wave_shr:1), as nw_pair_trace.hip does.  The strip's columns
// start at o(s) = s TR + 1 + lo, so a strip sweeps W + TR - 1 columns and never the whole row.  Cells
// off the band, left of column 1, right of column C or below row R are kept at minus infinity; column
// 0 and row 0 take their border values where the band holds them.
//
// The waves run in lockstep super-steps of 64 column steps with one __syncthreads() between them
// (nw_band_plan.h): strip s starts at super-step s lag, which puts the row it needs from strip s - 1
// into strictly earlier super-steps.  That row goes through a ring in LDS per wave, written by lane
// 63 and read by the consumer's lanes once per super-step, 64 columns at a time; within the super-step
// the values and the 64 subject letters (loaded a super-step ahead) come out of registers by
// v_readlane.  No wave polls anything: every loop is bounded by T, 64 and KR.
//
// With CODES the cells are kept as 4 v + tag and the fill stores nw_lanes_trace.h's 4-bit codes in
// this one pass, strip-major; without, plain int32 values and nothing but H(R, C) is stored.  The
// walk is nw_pair_trace.hip's one-lane loop with the strip's own column origin.  The bodies of the fill
// and of the walk are nw_band_dev.h's, which nw_band_batch.hip runs too.
#include "nw_band.h"

#include "nw_band_dev.h"
#include "nw_lanes_trace.h"
#include "nw_strip.h"

namespace gsa {

namespace {

template <bool AFFINE, bool CODES>
__global__ __launch_bounds__(64 * kBandWaves) void nw_band_kernel(const BandDesc* descs, const int* subst, int ssz, int go,
                                                                   int ge)
{
    __shared__ int tab[32 * 32];
    __shared__ int2 ring[kBandWaves][band_dev::RQ][64];
    band_dev::band_load_tab<CODES>(tab, subst, ssz);
    __syncthreads();
    const BandDesc d = descs[blockIdx.x];
    band_dev::band_pair_fill<AFFINE, CODES>(d, tab, &ring[0][0][0], ssz, go, ge);
}

// One lane (band_dev::band_walk).
__global__ __launch_bounds__(64) void nw_band_walk_kernel(BandWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    band_dev::band_walk(a);
}

template <bool AFFINE, bool CODES>
hipError_t launch_fill(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                       hipStream_t st)
{
    auto kern = nw_band_kernel<AFFINE, CODES>;
    hipError_t e = record_foot((const void*)kern, 0, 64 * waves, npairs);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(npairs), dim3(64 * waves), 0, st, descs, subst, substsz, go, ge);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_band(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                       bool codes, const BandWalkArgs* w, hipEvent_t* ev, hipStream_t st)
{
    if (npairs < 1 || waves < 1 || waves > kBandWaves) return hipErrorInvalidValue;
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
        hipLaunchKernelGGL(nw_band_walk_kernel, dim3(1), dim3(64), 0, st, *w);
        e = hipGetLastError();
    }
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
