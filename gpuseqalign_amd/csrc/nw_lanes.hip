// nw_lanes.hip -- database search, score-only NW / SW with linear or affine gaps: one query against
// many short subjects (gsa_score_db_dev).
//
// A wave task is kDbLanesSubj = 4 subjects, one per DPP row of 16 lanes.  Lane g of a row holds
// kDbLanesKQ = 24 consecutive query rows (H of the previous column, E in the affine modes, a best
// key per row in the local ones) in registers and walks the subject's columns one behind lane
// g - 1, whose last row it takes through a row_shr:1 DPP move: a wavefront of 16 lanes inside one
// wave, so no wave waits for another, there are no progress words and no spin loops.  One sweep
// covers 16 x 24 = 384 query rows; a longer query takes several sweeps, lane 15 leaving (H, F) of
// its last row per column in a per-wave boundary array that lane 0 of the next sweep reads.
// Lanes outside their subject's columns (the skew, a shorter subject in the same wave) are masked
// by EXEC, so nothing right of a subject's last column is ever computed.
// The query profile tab[d][i] = subst[query[i + 1]][d] (int32) is built once per workgroup in LDS;
// a lane reads its 24 values of a column with six ds_read_b128 at its own letter's row.
// Plain int32 Gotoh in the form of oracle/score_oracle.c; the linear modes keep no E / F (go == ge:
// H = max(diag + s, left + g, up + g)).
#include "nw_lanes.h"

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

template <bool LOCAL, bool AFFINE>
__global__ __launch_bounds__(64 * kDbLanesWaves) void nw_dblanes_kernel(DbLanesArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int tab[];
    const int Rpad = a.passes * kDbLanesPassRows;
    const int stride = Rpad + 4;  // = 4 (mod 8) dwords: rows of different letters start on different banks
    for (int idx = threadIdx.x; idx < a.substsz * Rpad; idx += blockDim.x)
    {
        const int d = idx / Rpad, i = idx - d * Rpad;
        // rows past the query: never the result row, and with NEG never above a real cell (local)
        tab[d * stride + i] = i < a.R ? a.subst[a.query[i + 1] * a.substsz + d] : kNeg;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int g = lane & (G - 1), grp = lane / G;
    const int slot = (blockIdx.x * kDbLanesWaves + (threadIdx.x >> 6)) * kDbLanesSubj + grp;
    const int go = a.go, ge = a.ge;
    int2* const bnd = a.bnd + (size_t)slot * (size_t)a.bndStride;
    // the lane and register row of the global result cell (R, C)
    const int gR = ((a.R - 1) % kDbLanesPassRows) / KQ, kR = (a.R - 1) % KQ;

    for (;;)
    {
        unsigned t = 0;
        if (lane == 0) t = atomicAdd(a.counter, 1u);
        t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= (unsigned)a.ntasks) break;
        const int s = (int)t * kDbLanesSubj + grp;
        const bool have = s < a.nsubj;
        const int C = have ? a.len[s] : 0;
        const int* const x = a.db + (have ? a.off[s] : 0ll);
        const int Cmax = max(max(__builtin_amdgcn_readlane(C, 0), __builtin_amdgcn_readlane(C, 16)),
                             max(__builtin_amdgcn_readlane(C, 32), __builtin_amdgcn_readlane(C, 48)));
        int bestS = 0, bi = 0, bj = 0, result = 0;

        for (int p = 0; p < a.passes; ++p)
        {
            const int i0 = p * kDbLanesPassRows + g * KQ;  // this lane's rows: i0 + 1 .. i0 + KQ
            int Hp[KQ], E[KQ], rb[KQ];
#pragma unroll
            for (int k = 0; k < KQ; ++k)
            {
                Hp[k] = LOCAL ? 0 : go + (i0 + k) * ge;  // column 0
                E[k] = kNeg;
                rb[k] = 0;
            }
            int hdiag = (LOCAL || i0 == 0) ? 0 : go + (i0 - 1) * ge;  // H(i0, 0)
            int fLast = kNeg;
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
                if (p == 0)
                {
                    above.x = LOCAL ? 0 : go + (j - 1) * ge;  // the border row
                    above.y = kNeg;
                }
                const int hu0 = from_lane_above(above.x, Hp[KQ - 1]);
                const int fu0 = AFFINE ? from_lane_above(above.y, fLast) : 0;
                if (j >= 1 && j <= C)
                {
                    const int4* const tr = reinterpret_cast<const int4*>(trow + let * stride);
                    const int jc = kDbLanesMaxC - j;
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
                            if (LOCAL) h = max(h, 0);
                            hdg = hp;
                            Hp[k] = h;
                            hup = h;
                            if (LOCAL) rb[k] = max(rb[k], (int)(((unsigned)h << kDbLanesJBits) | (unsigned)jc));
                        }
                    }
                    fLast = fup;
                    hdiag = hu0;
                    if (writes) bnd[j] = make_int2(hup, fup);
                }
            }
            if (LOCAL)
            {
                // rows in ascending order, a later one only when strictly better: first in row-major order
#pragma unroll
                for (int k = 0; k < KQ; ++k)
                {
                    const int hk = rb[k] >> kDbLanesJBits;
                    if (hk > bestS)
                    {
                        bestS = hk;
                        bi = i0 + 1 + k;
                        bj = kDbLanesMaxC - (rb[k] & kDbLanesMaxC);
                    }
                }
            }
            else if (p + 1 == a.passes)
            {
#pragma unroll
                for (int k = 0; k < KQ; ++k)
                    if (k == kR) result = Hp[k];
            }
            // the next sweep's lane 0 reads what this sweep's lane 15 wrote
            if (p + 1 < a.passes) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        }
        if (LOCAL)
        {
            // the 16 lanes of a subject hold disjoint rows: the best score, then the smallest row
#pragma unroll
            for (int m = G / 2; m >= 1; m >>= 1)
            {
                const int s2 = __shfl_xor(bestS, m), i2 = __shfl_xor(bi, m), j2 = __shfl_xor(bj, m);
                if (s2 > bestS || (s2 == bestS && s2 > 0 && i2 < bi))
                {
                    bestS = s2;
                    bi = i2;
                    bj = j2;
                }
            }
            if (have && g == 0) a.out[s] = DbLanesOut {bestS, bi, bj, 0};
        }
        else if (have && g == gR)
            a.out[s] = DbLanesOut {result, a.R, C, 0};
    }
}

template <bool LOCAL, bool AFFINE>
hipError_t prepare(size_t lds, int* wgs)
{
    auto kern = nw_dblanes_kernel<LOCAL, AFFINE>;
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

template <bool LOCAL, bool AFFINE>
hipError_t launch(const DbLanesArgs& a, int grid, hipStream_t st)
{
    auto kern = nw_dblanes_kernel<LOCAL, AFFINE>;
    const size_t lds = dblanes_lds_bytes(a.R, a.substsz);
    hipError_t e = record_foot((const void*)kern, lds, 64 * kDbLanesWaves, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kDbLanesWaves), lds, st, a);
    return hipGetLastError();
}

}  // namespace

size_t dblanes_lds_bytes(int R, int substsz)
{
    const size_t passes = ((size_t)R + kDbLanesPassRows - 1) / kDbLanesPassRows;
    return (size_t)substsz * (passes * kDbLanesPassRows + 4) * sizeof(int);
}

hipError_t dblanes_resident(int R, int substsz, int local, bool affine, int* wgs)
{
    const size_t lds = dblanes_lds_bytes(R, substsz);
    if (local) return affine ? prepare<true, true>(lds, wgs) : prepare<true, false>(lds, wgs);
    return affine ? prepare<false, true>(lds, wgs) : prepare<false, false>(lds, wgs);
}

hipError_t launch_dblanes(const DbLanesArgs& a, int local, int grid, int* gridOut, hipStream_t st)
{
    const bool affine = a.go != a.ge;
    if (grid <= 0)
    {
        int wgs = 1;
        hipError_t e = dblanes_resident(a.R, a.substsz, local, affine, &wgs);
        if (e != hipSuccess) return e;
        grid = std::max(1, std::min(wgs, (a.ntasks + kDbLanesWaves - 1) / kDbLanesWaves));
    }
    if (gridOut) *gridOut = grid;
    if (local) return affine ? launch<true, true>(a, grid, st) : launch<true, false>(a, grid, st);
    return affine ? launch<false, true>(a, grid, st) : launch<false, false>(a, grid, st);
}

}  // namespace gsa
