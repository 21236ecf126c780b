// nw_lanes_semi.hip -- database search, score-only, semi-global with linear or affine gaps: the whole
// query within each subject, the subject's head and tail free (gsa_score_db_multi_semi_dev;
// DESIGN.md 2.2h).
//
// Row 0 is free (H(0, j) = 0, no E / F there), column 0 is the global one (H(i, 0) = go + (i - 1) ge),
// and the result is the best H of row R, at the smallest column that attains it; column 0, the
// all-insert alignment, is a candidate.  No zero floor: scores may be negative.
//
// The schedule is nw_lanes_multi.hip's (units of kDbMultiUnit wave tasks of one query, claimed by a
// workgroup through LDS, the profile rebuilt when the query changes, one launch per sweep class, the
// per-wave boundary array between sweeps, results in subject order), and so is the per-cell code.
// The layout differs: the query is aligned to the BOTTOM of the sweep grid.  A launch's queries all
// take `passes` sweeps of 384 rows; a query of R letters has pad = passes * 384 - R < 384 padding rows
// ABOVE its row 1, all in the first sweep.  A padding row has profile value 0, column 0 equal to 0 and
// starts with E = minus infinity, so every padding cell is H = max(0 + 0, go, go) = 0 and hands down
// F = go: the padding rows stand in for row 0 exactly (F(1, j) = max(go + ge, 0 + go) = go, as the true
// border gives; in the linear instances only H = 0 is handed down).  Row R is then always the last
// register row of lane 15 in the last sweep, whatever R is, and tracking it costs one key and one
// max per step, not per cell.  The key is signed: H * 2^13 + (8191 - j), which |H| < 2^18 allows.
// Nothing here waits on anything but __syncthreads(): no spin loops, no progress words; every loop is
// bounded by C + 15, the sweep count or the task count.
#include "nw_lanes_semi.h"

#include <algorithm>

#include "nw_strip.h"

namespace gsa {

namespace {

constexpr int G = kDbLanesG;
constexpr int KQ = kDbLanesKQ;
constexpr int kNeg = -(1 << 29);

__device__ __forceinline__ int from_lane_above(int own, int src)
{
    // row_shr:1 within the 16 lanes of a subject; lane 0 of a row has no source and keeps `own`
    return __builtin_amdgcn_update_dpp(own, src, 0x111, 0xf, 0xf, false);
}

__device__ __forceinline__ int row_key(int h, int j)
{
    // ordered by (h, smaller j first) as a signed int; |h| < 2^18, 0 <= j <= 8191
    return (int)(((unsigned)h << kDbLanesJBits) | (unsigned)(kDbLanesMaxC - j));
}

template <bool AFFINE>
__global__ __launch_bounds__(64 * kDbLanesWaves) void nw_dbsemi_kernel(DbMultiArgs a)
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
        const int key0 = row_key(go + (R - 1) * ge, 0);  // the all-insert alignment, H(R, 0)

        for (int t = ub * kDbMultiUnit + wave; t < tEnd; t += kDbLanesWaves)
        {
            const int s = t * kDbLanesSubj + grp;
            const bool have = s < a.nsubj;
            const int C = have ? a.len[s] : 0;
            const int* const x = a.db + (have ? a.off[s] : 0ll);
            const int Cmax = max(max(__builtin_amdgcn_readlane(C, 0), __builtin_amdgcn_readlane(C, 16)),
                                 max(__builtin_amdgcn_readlane(C, 32), __builtin_amdgcn_readlane(C, 48)));
            int best = key0;

            for (int p = 0; p < a.passes; ++p)
            {
                const int i0 = p * kDbLanesPassRows + g * KQ;  // this lane's grid rows: i0 + 1 .. i0 + KQ
                const int q0 = i0 - pad;                       // its query rows: q0 + 1 .. q0 + KQ (<= 0: padding)
                int Hp[KQ], E[KQ];
#pragma unroll
                for (int k = 0; k < KQ; ++k)
                {
                    Hp[k] = q0 + k >= 0 ? go + (q0 + k) * ge : 0;  // column 0
                    E[k] = kNeg;
                }
                int hdiag = q0 >= 1 ? go + (q0 - 1) * ge : 0;  // H(q0, 0)
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
                        best = max(best, row_key(hup, j));
                    }
                }
                // the next sweep's lane 0 reads what this sweep's lane 15 wrote
                if (p + 1 < a.passes) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            }
            if (have && g == G - 1)
                orow[a.sidx[s]] = DbLanesOut {best >> kDbLanesJBits, R, kDbLanesMaxC - (best & kDbLanesMaxC), 0};
        }
    }
}

template <bool AFFINE>
hipError_t prepare(size_t lds, int* wgs)
{
    auto kern = nw_dbsemi_kernel<AFFINE>;
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
    auto kern = nw_dbsemi_kernel<AFFINE>;
    const size_t lds = dbmulti_lds_bytes(a.passes, a.substsz);
    hipError_t e = record_foot((const void*)kern, lds, 64 * kDbLanesWaves, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kDbLanesWaves), lds, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t dbsemi_resident(int passes, int substsz, bool affine, int* wgs)
{
    const size_t lds = dbmulti_lds_bytes(passes, substsz);
    return affine ? prepare<true>(lds, wgs) : prepare<false>(lds, wgs);
}

hipError_t launch_dbsemi(const DbMultiArgs& a, int grid, hipStream_t st)
{
    return a.go != a.ge ? launch<true>(a, grid, st) : launch<false>(a, grid, st);
}

}  // namespace gsa
