// nw_lanes_overlap.hip -- database search, score-only, overlap (dovetail) with linear or affine gaps:
// a suffix of either sequence on a prefix of the other, or either within the other
// (gsa_score_db_multi_overlap_dev).
//
// Row 0 and column 0 are free (H = 0, no E / F there), and the result is the best H among row R
// (j = 0 ... C) and column C (i = 0 ... R): (R, smallest j) if row R attains it, else (smallest i, C).
// No zero floor inside, but the score is never negative: H(R, 0) = 0 is a candidate.
//
// The schedule, the per-cell code and the bottom-aligned layout are nw_lanes_semi.hip's: a query of R
// letters has pad = passes * 384 - R < 384 padding rows above its row 1, all in the first sweep.  A
// padding row has profile value 0, column 0 equal to 0 and starts with E = minus infinity, so every
// padding cell is H = max(0 + 0, go, go) = 0 and hands down F = go, as the free row 0 does.  Row R is
// the last register row of lane 15 in the last sweep, tracked by one key and one max per step.
// What differs:
//   column 0: every lane's rows start from H(i, 0) = 0, and the diagonal into column 1 is 0;
//   column C: in every sweep a lane stands on column C at step C + g with its 24 rows' H in
//   registers, and no later step of the sweep touches them (the per-cell code runs for j <= C only).
//   So the fold needs no branch in the step loop: behind the loop, once per lane and sweep, every
//   lane's registers hold column C, whichever C its 16-lane group has and however early its step
//   C + g fell.  It folds them into a running best ordered by (value, smaller i first).  Within the
//   fold the key is H * 2^5 + (23 - k); the winner goes into the signed key H * 2^13 + (8191 - i)
//   that lives across sweeps.  (With the fold behind a branch at step C + g, the wave ran it at up to
//   64 different steps per sweep; the linear instance measured 6 % above the semi-global one.)
//   Padding rows are folded too: they
//   hold 0, and a column value wins only when it is greater than row R's, which is >= 0; their row
//   index is clamped to 0 so the key does not overflow.  After the last sweep the 16 lanes of a
//   subject reduce their keys by four row rotations (DPP), and lane 15 combines row and column.
// The keys need |H| < 2^18 and R, C <= 8191, which the host tests before the launch.
// Nothing here waits on anything but __syncthreads(): no spin loops, no progress words; every loop is
// bounded by C + 15, the sweep count or the task count.
#include "nw_lanes_overlap.h"

#include <algorithm>

#include "nw_strip.h"

namespace gsa {

namespace {

constexpr int G = kDbLanesG;
constexpr int KQ = kDbLanesKQ;
constexpr int kNeg = -(1 << 29);
constexpr int kStepBits = 5;  // a step's key: H * 2^5 + (23 - k)

__device__ __forceinline__ int from_lane_above(int own, int src)
{
    // row_shr:1 within the 16 lanes of a subject; lane 0 of a row has no source and keeps `own`
    return __builtin_amdgcn_update_dpp(own, src, 0x111, 0xf, 0xf, false);
}

template <int N>
__device__ __forceinline__ int row_rotated(int v)
{
    // row_ror:N within the 16 lanes of a subject
    return __builtin_amdgcn_update_dpp(v, v, 0x120 + N, 0xf, 0xf, false);
}

__device__ __forceinline__ int cell_key(int h, int at)
{
    // ordered by (h, smaller position first) as a signed int; |h| < 2^18, 0 <= at <= 8191
    return (int)(((unsigned)h << kDbLanesJBits) | (unsigned)(kDbLanesMaxC - at));
}

template <bool AFFINE>
__global__ __launch_bounds__(64 * kDbLanesWaves) void nw_dboverlap_kernel(DbMultiArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int tab[];
    __shared__ unsigned claimed;
    const int Rpad = a.passes * kDbLanesPassRows;
    const int stride = Rpad + 4;  // = 4 (mod 8) dwords: rows of different letters start on different banks
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = lane & (G - 1), grp = lane / G;
    const int slot = (blockIdx.x * kDbLanesWaves + wave) * kDbLanesSubj + grp;
    const int go = a.go, ge = a.ge;
    int2* const bnd = a.bnd + (size_t)slot * (size_t)a.bndStride;
    int resident = -1;  // the query whose profile is in LDS (workgroup-uniform)

    for (;;)
    {
        // every wave is done with the last unit's profile and has read the last claim
        __syncthreads();
        if (threadIdx.x == 0) claimed = atomicAdd(a.counter, 1u);
        __syncthreads();
        const int u = __builtin_amdgcn_readfirstlane((int)claimed);
        if (u >= a.nunits) break;  // the same word for all threads of the workgroup
        const int ql = u / a.unitsPerQuery, ub = u - ql * a.unitsPerQuery;
        const DbMultiQuery qd = a.q[ql];
        const int R = qd.R;
        const int pad = Rpad - R;  // padding rows above row 1: 0 ... 383, all in the first sweep
        if (ql != resident)
        {
            const int* const query = a.queries + qd.off;
            for (int idx = threadIdx.x; idx < a.substsz * Rpad; idx += blockDim.x)
            {
                const int d = idx / Rpad, r = idx - d * Rpad;
                // grid row r + 1 is query row r + 1 - pad; a padding row scores 0 against every letter
                tab[d * stride + r] = r >= pad ? a.subst[query[r - pad + 1] * a.substsz + d] : 0;
            }
            if (threadIdx.x == 0) atomicAdd(a.builds, 1u);
            resident = ql;
            __syncthreads();
        }
        DbLanesOut* const orow = a.out + (size_t)qd.row * (size_t)a.ld;
        const int tEnd = min((ub + 1) * kDbMultiUnit, a.ntasks);
        const int key0 = cell_key(0, 0);  // H(R, 0) = 0; as a column key, H(0, C) = 0

        for (int t = ub * kDbMultiUnit + wave; t < tEnd; t += kDbLanesWaves)
        {
            const int s = t * kDbLanesSubj + grp;
            const bool have = s < a.nsubj;
            const int C = have ? a.len[s] : 0;
            const int* const x = a.db + (have ? a.off[s] : 0ll);
            const int Cmax = max(max(__builtin_amdgcn_readlane(C, 0), __builtin_amdgcn_readlane(C, 16)),
                                 max(__builtin_amdgcn_readlane(C, 32), __builtin_amdgcn_readlane(C, 48)));
            int best = key0;     // row R: (value, smaller j first)
            int colBest = key0;  // column C over all sweeps: (value, smaller i first)

            for (int p = 0; p < a.passes; ++p)
            {
                const int i0 = p * kDbLanesPassRows + g * KQ;  // this lane's grid rows: i0 + 1 .. i0 + KQ
                const int q0 = i0 - pad;                       // its query rows: q0 + 1 .. q0 + KQ (<= 0: padding)
                int Hp[KQ], E[KQ];
#pragma unroll
                for (int k = 0; k < KQ; ++k)
                {
                    Hp[k] = 0;  // column 0 is free
                    E[k] = kNeg;
                }
                int hdiag = 0;  // H(q0, 0)
                int fLast = kNeg;
                best = key0;  // the last sweep's is the result
                const bool reads = p > 0 && g == 0, writes = p + 1 < a.passes && g == G - 1;
                // the letter and the row above of the next step, loaded one step ahead
                int letNext = (1 - g >= 1 && 1 - g <= C) ? x[1 - g] : 0;
                int2 bndNext = make_int2(0, kNeg);
                if (reads && C >= 1) bndNext = bnd[1];
                const int* const trow = tab + i0;

                for (int step = 1; step <= Cmax + G - 1; ++step)
                {
                    const int j = step - g;
                    const int let = letNext;
                    int2 above = bndNext;
                    if (j + 1 >= 1 && j + 1 <= C)
                    {
                        letNext = x[j + 1];
                        if (reads) bndNext = bnd[j + 1];
                    }
                    if (p == 0) above = make_int2(0, kNeg);  // the free row 0
                    const int hu0 = from_lane_above(above.x, Hp[KQ - 1]);
                    const int fu0 = AFFINE ? from_lane_above(above.y, fLast) : 0;
                    if (j >= 1 && j <= C)
                    {
                        const int4* const tr = reinterpret_cast<const int4*>(trow + let * stride);
                        int hup = hu0, fup = fu0, hdg = hdiag;
#pragma unroll
                        for (int q = 0; q < KQ / 4; ++q)
                        {
                            const int4 sv = tr[q];
                            const int sk[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                            {
                                const int k = 4 * q + r;
                                const int hp = Hp[k];
                                int h;
                                if (AFFINE)
                                {
                                    const int e = max(E[k] + ge, hp + go);
                                    const int f = max(fup + ge, hup + go);
                                    h = max(max(hdg + sk[r], e), f);
                                    E[k] = e;
                                    fup = f;
                                }
                                else
                                    h = max(max(hdg + sk[r], hp + go), hup + go);
                                hdg = hp;
                                Hp[k] = h;
                                hup = h;
                            }
                        }
                        fLast = fup;
                        hdiag = hu0;
                        if (writes) bnd[j] = make_int2(hup, fup);
                        // the lane's last row inside its own columns; lane 15's in the last sweep is row R
                        best = max(best, cell_key(hup, j));
                    }
                }
                {
                    // Column C, once per lane and sweep: a lane's rows are not touched after its step C + g, so
                    // behind the loop Hp is column C in every lane, whatever C its group has (no subject: 0s).
                    int m = (int)(((unsigned)Hp[0] << kStepBits) | (unsigned)(KQ - 1));
#pragma unroll
                    for (int k = 1; k < KQ; ++k)
                        m = max(m, (int)(((unsigned)Hp[k] << kStepBits) | (unsigned)(KQ - 1 - k)));
                    const int k = KQ - 1 - (m & ((1 << kStepBits) - 1));
                    // a padding row (value 0, never the result) stands at row 0
                    colBest = max(colBest, cell_key(m >> kStepBits, max(q0 + k + 1, 0)));
                }
                // the next sweep's lane 0 reads what this sweep's lane 15 wrote
                if (p + 1 < a.passes) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            }
            // column C over the subject's 16 lanes: every lane gets the best key
            colBest = max(colBest, row_rotated<8>(colBest));
            colBest = max(colBest, row_rotated<4>(colBest));
            colBest = max(colBest, row_rotated<2>(colBest));
            colBest = max(colBest, row_rotated<1>(colBest));
            if (have && g == G - 1)
            {
                const int rowV = best >> kDbLanesJBits, colV = colBest >> kDbLanesJBits;
                orow[a.sidx[s]] = rowV >= colV ? DbLanesOut {rowV, R, kDbLanesMaxC - (best & kDbLanesMaxC), 0}
                                               : DbLanesOut {colV, kDbLanesMaxC - (colBest & kDbLanesMaxC), C, 0};
            }
        }
    }
}

template <bool AFFINE>
hipError_t prepare(size_t lds, int* wgs)
{
    auto kern = nw_dboverlap_kernel<AFFINE>;
    hipError_t e = hipSuccess;
    if (lds > 65536)
        e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    int per_cu = 0, dev = 0, cus = 0;
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * kDbLanesWaves, lds);
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) *wgs = std::max(1, per_cu) * std::max(1, cus);
    return e;
}

template <bool AFFINE>
hipError_t launch(const DbMultiArgs& a, int grid, hipStream_t st)
{
    auto kern = nw_dboverlap_kernel<AFFINE>;
    const size_t lds = dbmulti_lds_bytes(a.passes, a.substsz);
    hipError_t e = record_foot((const void*)kern, lds, 64 * kDbLanesWaves, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kDbLanesWaves), lds, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t dboverlap_resident(int passes, int substsz, bool affine, int* wgs)
{
    const size_t lds = dbmulti_lds_bytes(passes, substsz);
    return affine ? prepare<true>(lds, wgs) : prepare<false>(lds, wgs);
}

hipError_t launch_dboverlap(const DbMultiArgs& a, int grid, hipStream_t st)
{
    return a.go != a.ge ? launch<true>(a, grid, st) : launch<false>(a, grid, st);
}

}  // namespace gsa
