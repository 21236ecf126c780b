// nw_lanes_multi.hip -- database search, score-only NW / SW with linear or affine gaps: many queries
// against many short subjects in one persistent launch (gsa_score_db_multi_dev).
//
// The layout and the per-cell code are nw_lanes.hip's (a subject per DPP row of 16 lanes, 24 query
// rows per lane, the row_shr:1 hand-off, EXEC masking, sweeps of 384 rows over a per-wave boundary
// array, a best key per row in the local modes), restated here so that nw_lanes.hip and its four
// instances stay as they are.  What is new: the query profile in LDS changes during the launch.
// The work is cut into units, one query and kDbMultiUnit consecutive wave tasks of it, ordered
// query-major; a WORKGROUP claims a unit (one thread's atomicAdd, broadcast through LDS), rebuilds the
// profile when the unit's query is not the resident one, and its four waves take the unit's tasks
// round-robin.  The claim and the exit test are read from LDS behind a barrier, so every wave of a
// workgroup meets every barrier the same number of times; the barrier at the top of the loop keeps a
// fast wave from overwriting a profile another wave still reads.  Nothing here waits on anything but
// __syncthreads(): no spin loops, no progress words, no wave waiting for another workgroup.
// The result of (query, subject) goes to out[row * ld + subject], in subject order, so the matrix is
// ranked and copied without a permutation; the ranking (segmented radix sort of
// score << 32 | ~subject keys, hipCUB) and the small kernels around it are at the end of this file.
#include "nw_lanes_multi.h"

#include <algorithm>

#include <hipcub/hipcub.hpp>

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
__global__ __launch_bounds__(64 * kDbLanesWaves) void nw_dbmulti_kernel(DbMultiArgs a)
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
        if (ql != resident)
        {
            const int* const query = a.queries + qd.off;
            for (int idx = threadIdx.x; idx < a.substsz * Rpad; idx += blockDim.x)
            {
                const int d = idx / Rpad, i = idx - d * Rpad;
                // rows past the query: never the result row, and with NEG never above a real cell (local)
                tab[d * stride + i] = i < R ? a.subst[query[i + 1] * a.substsz + d] : kNeg;
            }
            if (threadIdx.x == 0) atomicAdd(a.builds, 1u);
            resident = ql;
            __syncthreads();
        }
        // the lane and register row of the global result cell (R, C)
        const int gR = ((R - 1) % kDbLanesPassRows) / KQ, kR = (R - 1) % KQ;
        DbLanesOut* const orow = a.out + (size_t)qd.row * (size_t)a.ld;
        const int tEnd = min((ub + 1) * kDbMultiUnit, a.ntasks);

        for (int t = ub * kDbMultiUnit + wave; t < tEnd; t += kDbLanesWaves)
        {
            const int s = t * kDbLanesSubj + grp;
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
                    // Hp[kR] by the bits of kR: five masks, not one per row
                    int v[32];
#pragma unroll
                    for (int k = 0; k < 32; ++k) v[k] = k < KQ ? Hp[k] : 0;
#pragma unroll
                    for (int b = 0; b < 5; ++b)
                    {
                        const bool odd = (kR >> b) & 1;
#pragma unroll
                        for (int k = 0; k < (16 >> b); ++k) v[k] = odd ? v[2 * k + 1] : v[2 * k];
                    }
                    result = v[0];
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
                if (have && g == 0) orow[a.sidx[s]] = DbLanesOut {bestS, bi, bj, 0};
            }
            else if (have && g == gR)
                orow[a.sidx[s]] = DbLanesOut {result, R, C, 0};
        }
    }
}

template <bool LOCAL, bool AFFINE>
hipError_t prepare(size_t lds, int* wgs)
{
    auto kern = nw_dbmulti_kernel<LOCAL, AFFINE>;
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
hipError_t launch(const DbMultiArgs& a, int grid, hipStream_t st)
{
    auto kern = nw_dbmulti_kernel<LOCAL, AFFINE>;
    const size_t lds = dbmulti_lds_bytes(a.passes, a.substsz);
    hipError_t e = record_foot((const void*)kern, lds, 64 * kDbLanesWaves, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kDbLanesWaves), lds, st, a);
    return hipGetLastError();
}

__global__ void dbmulti_scatter_kernel(const DbMultiPatch* list, long long n, DbLanesOut* out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[list[k].index] = list[k].v;
}

__global__ void dbmulti_scores_kernel(const DbLanesOut* out, long long n, int* scores)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) scores[k] = out[k].score;
}

// key = score << 32 | (2^32 - 1 - subject): descending keys are (score descending, subject ascending)
__global__ void dbmulti_keys_kernel(const DbLanesOut* out, int nq, int nsubj, long long* keys, int* seg)
{
    const long long n = (long long)nq * nsubj;
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= nq) seg[k] = (int)(k * nsubj);
    if (k >= n) return;
    const unsigned s = (unsigned)(k % nsubj);
    keys[k] = (long long)(((unsigned long long)(unsigned)out[k].score << 32) | (unsigned long long)(0xFFFFFFFFu - s));
}

__global__ void dbmulti_hits_kernel(const DbLanesOut* out, const long long* sorted, int nq, int nsubj, int ntop,
                                    DbMultiHit* hits)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)nq * ntop) return;
    const long long q = k / ntop, r = k - q * ntop;
    const unsigned s = 0xFFFFFFFFu - (unsigned)((unsigned long long)sorted[q * nsubj + r] & 0xFFFFFFFFull);
    const DbLanesOut o = out[q * nsubj + s];
    hits[k] = DbMultiHit {(int)s, o.score, o.i_end, o.j_end};
}

constexpr int kSmall = 256;
inline unsigned blocks_of(long long n) { return (unsigned)((n + kSmall - 1) / kSmall); }
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

size_t dbmulti_lds_bytes(int passes, int substsz)
{
    return (size_t)substsz * ((size_t)passes * kDbLanesPassRows + 4) * sizeof(int);
}

hipError_t dbmulti_resident(int passes, int substsz, int local, bool affine, int* wgs)
{
    const size_t lds = dbmulti_lds_bytes(passes, substsz);
    if (local) return affine ? prepare<true, true>(lds, wgs) : prepare<true, false>(lds, wgs);
    return affine ? prepare<false, true>(lds, wgs) : prepare<false, false>(lds, wgs);
}

hipError_t launch_dbmulti(const DbMultiArgs& a, int local, int grid, hipStream_t st)
{
    const bool affine = a.go != a.ge;
    if (local) return affine ? launch<true, true>(a, grid, st) : launch<true, false>(a, grid, st);
    return affine ? launch<false, true>(a, grid, st) : launch<false, false>(a, grid, st);
}

hipError_t launch_dbmulti_scatter(const DbMultiPatch* list, long long n, DbLanesOut* out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(dbmulti_scatter_kernel, dim3(blocks_of(n)), dim3(kSmall), 0, st, list, n, out);
    return hipGetLastError();
}

hipError_t launch_dbmulti_scores(const DbLanesOut* out, long long n, int* scores, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(dbmulti_scores_kernel, dim3(blocks_of(n)), dim3(kSmall), 0, st, out, n, scores);
    return hipGetLastError();
}

hipError_t dbmulti_select_bytes(int nq, int nsubj, size_t* bytes, size_t* tempBytes)
{
    const long long n = (long long)nq * nsubj;
    size_t temp = 0;
    const hipError_t e = hipcub::DeviceSegmentedRadixSort::SortKeysDescending(
        nullptr, temp, (const long long*)nullptr, (long long*)nullptr, (int)n, nq, (const int*)nullptr,
        (const int*)nullptr);
    if (e != hipSuccess) return e;
    *tempBytes = temp;
    *bytes = 2 * up256((size_t)n * sizeof(long long)) + up256(((size_t)nq + 1) * sizeof(int)) + up256(temp);
    return hipSuccess;
}

hipError_t launch_dbmulti_select(const DbLanesOut* out, int nq, int nsubj, int ntop, void* scratch, size_t tempBytes,
                                 DbMultiHit* hits, hipStream_t st)
{
    const long long n = (long long)nq * nsubj;
    char* const base = (char*)scratch;
    long long* const keys = (long long*)base;
    long long* const sorted = (long long*)(base + up256((size_t)n * sizeof(long long)));
    int* const seg = (int*)(base + 2 * up256((size_t)n * sizeof(long long)));
    void* const temp = (char*)seg + up256(((size_t)nq + 1) * sizeof(int));
    hipLaunchKernelGGL(dbmulti_keys_kernel, dim3(blocks_of(n + 1)), dim3(kSmall), 0, st, out, nq, nsubj, keys, seg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = tempBytes;
    e = hipcub::DeviceSegmentedRadixSort::SortKeysDescending(temp, tb, (const long long*)keys, sorted, (int)n, nq,
                                                             (const int*)seg, (const int*)seg + 1, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dbmulti_hits_kernel, dim3(blocks_of((long long)nq * ntop)), dim3(kSmall), 0, st, out, sorted, nq,
                       nsubj, ntop, hits);
    return hipGetLastError();
}

}  // namespace gsa
