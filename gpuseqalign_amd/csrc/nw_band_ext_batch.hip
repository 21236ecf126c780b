// nw_band_ext_batch.hip -- the banded extension calls over a batch of long pairs
// (gsa_score_band_ext_batch_dev, gsa_align_batch_band_ext_dev).
//
// The fill is nw_band_batch.hip's persistent grid: a workgroup claims the next pair from one counter --
// one atomicAdd by thread 0, handed to the other threads through LDS behind a __syncthreads() -- and
// runs the pair's lockstep super-steps in the extension mode (nw_band_dev.h), until the counter passes
// the pair count.  band_pair_fill sets all per-strip state and the best values anew per pair; the
// barrier at the top of the claim loop stands between thread 0's read of the waves' slots and the next
// pair's first write to them, as it does for the ring.  Nothing polls memory, there is no spin loop and
// no hand-off between workgroups: the claim loop is bounded by the pair count, the loops of the body by
// T, 64, KR and the waves; the claim is the only atomic.
//
// The workgroup has 4, 8 or 16 waves (nw_band_batch_plan.h); the ring is dynamic LDS, the slots of the
// best cells are 16 x 16 bytes beside the table.
//
// The walks take one wave per pair (lane 0 walks, band_dev::band_walk, from the pair's end cell),
// grid-strided when the grid is capped; every pair has its own record and move bytes.
#include "nw_band_ext_batch.h"

#include <algorithm>

#include "nw_band_dev.h"
#include "nw_strip.h"

namespace gsa {

namespace {

inline size_t ring_bytes(int waves) { return (size_t)waves * band_dev::RQ * 64 * sizeof(int2); }

template <bool AFFINE, bool CODES>
__global__ __launch_bounds__(64 * kBandWaves) void nw_band_ext_batch_kernel(const BandDesc* __restrict__ descs, int npairs,
                                                                             unsigned* counter, const int* subst, int ssz, int go,
                                                                             int ge)
{
    __shared__ int tab[32 * 32];
    __shared__ int4 best[kBandWaves];
    __shared__ unsigned claim;
    extern __shared__ int2 ring[];  // [waves][RQ][64]
    band_dev::band_load_tab<CODES>(tab, subst, ssz);
    for (int it = 0; it < npairs; ++it)
    {
        // behind the table's load; behind every read of `claim`, of the ring and of `best` by the pair before
        __syncthreads();
        if (threadIdx.x == 0) claim = atomicAdd(counter, 1u);
        __syncthreads();
        // the same value in every lane: the descriptor and all that follows from it stay in scalar registers
        const unsigned p = (unsigned)__builtin_amdgcn_readfirstlane((int)claim);
        if (p >= (unsigned)npairs) break;
        const BandDesc d = descs[p];
        band_dev::band_pair_fill<AFFINE, CODES, true>(d, tab, ring, ssz, go, ge, best);
    }
}

// One wave per pair, lane 0 walks.
__global__ __launch_bounds__(64) void nw_band_ext_batch_walk_kernel(const BandWalkArgs* walks, int nwalks)
{
    if (threadIdx.x != 0) return;
    for (int q = blockIdx.x; q < nwalks; q += gridDim.x)
    {
        const BandWalkArgs a = walks[q];
        band_dev::band_walk_from_start(a);
    }
}

template <bool AFFINE, bool CODES>
hipError_t fill_grid(int waves, int npairs, int maxWgs, int* grid)
{
    auto kern = nw_band_ext_batch_kernel<AFFINE, CODES>;
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * waves, ring_bytes(waves));
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    int g = std::max(1, std::min(npairs, std::max(1, per_cu) * std::max(1, cus)));
    if (maxWgs > 0) g = std::min(g, maxWgs);
    *grid = g;
    return hipSuccess;
}

template <bool AFFINE, bool CODES>
hipError_t launch_fill(const BandDesc* descs, int npairs, unsigned* counter, int waves, int grid, const int* subst,
                       int substsz, int go, int ge, hipStream_t st)
{
    auto kern = nw_band_ext_batch_kernel<AFFINE, CODES>;
    hipError_t e = record_foot((const void*)kern, ring_bytes(waves), 64 * waves, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * waves), ring_bytes(waves), st, descs, npairs, counter, subst, substsz, go,
                       ge);
    return hipGetLastError();
}

}  // namespace

hipError_t band_ext_batch_fill_grid(bool affine, bool codes, int waves, int npairs, int maxWgs, int* grid)
{
    if (npairs < 1 || maxWgs < 0 || (waves != 4 && waves != 8 && waves != 16)) return hipErrorInvalidValue;
    return codes ? (affine ? fill_grid<true, true>(waves, npairs, maxWgs, grid) : fill_grid<false, true>(waves, npairs, maxWgs, grid))
                 : (affine ? fill_grid<true, false>(waves, npairs, maxWgs, grid)
                           : fill_grid<false, false>(waves, npairs, maxWgs, grid));
}

hipError_t launch_band_ext_batch(const BandDesc* descs, int npairs, unsigned* counter, int waves, int grid, const int* subst,
                                 int substsz, int go, int ge, bool codes, const BandWalkArgs* walks, int walkGrid,
                                 hipEvent_t* ev, hipStream_t st)
{
    if (npairs < 1 || grid < 1 || (waves != 4 && waves != 8 && waves != 16) || (walks && walkGrid < 1))
        return hipErrorInvalidValue;
    const bool affine = go != ge;
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[0], st);
    e = codes ? (affine ? launch_fill<true, true>(descs, npairs, counter, waves, grid, subst, substsz, go, ge, st)
                        : launch_fill<false, true>(descs, npairs, counter, waves, grid, subst, substsz, go, ge, st))
              : (affine ? launch_fill<true, false>(descs, npairs, counter, waves, grid, subst, substsz, go, ge, st)
                        : launch_fill<false, false>(descs, npairs, counter, waves, grid, subst, substsz, go, ge, st));
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    if (walks)
    {
        hipLaunchKernelGGL(nw_band_ext_batch_walk_kernel, dim3(walkGrid), dim3(64), 0, st, walks, npairs);
        e = hipGetLastError();
    }
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
