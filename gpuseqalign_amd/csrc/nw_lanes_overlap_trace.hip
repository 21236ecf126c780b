// nw_lanes_overlap_trace.hip -- database search, the overlap (dovetail) alignments of many queries'
// hits in one call (gsa_align_db_multi_overlap_dev): a suffix of either sequence on a
// prefix of the other, or either within the other, linear or affine gaps, traced on the device.
//
// The schedule, the per-cell code and the code format are nw_lanes_trace_multi.hip's (units of up to
// kDbAlignMultiUnit wave tasks of one query claimed by a workgroup through LDS, values kept as
// 4 v + tag, one maximum that picks a value and its source, a lane's 24 codes of a column in one
// 12-byte store at codes[hit] + ((sweep (C + 1) + j) 16 + g) 12), restated here as
// nw_lanes_semi_trace.hip restates them, so that the existing instances stay as they are.  The layout
// is the existing one too: the query at the top of the sweep grid, the padding rows below row R.
// The borders: the row above the first sweep is the free row 0 (H = 0, no F), and column 0 is H = 0,
// E = minus infinity in every row.
// The end cell is found on the tagged values.  Row R: in the last sweep every step picks Hp[kR] by
// the bits of kR (five masks) and folds it into one signed key, 4 H * 2^11 + (8191 - j), started at
// column 0's value 0.  Column C: a lane's rows are not touched after the step at which it stands on
// column C, so behind the step loop of every sweep its registers hold column C, and there it folds
// its rows i <= R into a key ordered by (value, smaller i first) -- within the fold
// 4 H * 2^3 + (23 - k), across sweeps 4 H * 2^11 + (8191 - i), started at row 0's value 0; the 16
// lanes of a hit reduce it by four row rotations (DPP).  Row R's cell is the result if its value is
// >= the column's, else the column's: the score kernel's end cell.
// The walk is nw_lanes_trace_multi.hip's with the exit at i = 0 or j = 0: it starts at (i_end, j_end)
// in whatever sweep that lies, and nothing is emitted along a border.
// Nothing here waits on anything but __syncthreads(): no spin loops, no progress words.
#include "nw_lanes_overlap_trace.h"

#include <algorithm>

#include "nw_strip.h"

namespace gsa {

namespace {

constexpr int G = kDbLanesG;
constexpr int KQ = kDbLanesKQ;
constexpr int kNegQ = -(1 << 29);  // 4 x "minus infinity" (-2^27), tag 0
constexpr int kNoKey = -2147483647 - 1;
constexpr int kStepBits = 5;  // a step's key: H * 2^5 + (23 - k)
constexpr int kWalkThreads = 64;
constexpr unsigned kWalkH = 4u;  // the walk's state H; inside a gap the state is the gap's source code

struct __attribute__((aligned(4))) Codes3
{
    unsigned a, b, c;
};

__device__ __forceinline__ int from_lane_above(int own, int src)
{
    // row_shr:1 within the 16 lanes of a hit; lane 0 of a row has no source and keeps `own`
    return __builtin_amdgcn_update_dpp(own, src, 0x111, 0xf, 0xf, false);
}

template <int N>
__device__ __forceinline__ int row_rotated(int v)
{
    // row_ror:N within the 16 lanes of a hit
    return __builtin_amdgcn_update_dpp(v, v, 0x120 + N, 0xf, 0xf, false);
}

__device__ __forceinline__ int cell_key4(int h4, int back)
{
    // h4 = 4 H with tag 0, back = 8191 - position: H * 2^13 + back, ordered by (H, smaller position
    // first) as a signed int
    return (int)(((unsigned)h4 << (kDbLanesJBits - 2)) | (unsigned)back);
}

template <bool AFFINE>
__global__ __launch_bounds__(64 * kDbLanesWaves) void nw_dboverlap_fill_kernel(DbTraceMultiArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int tab[];
    __shared__ unsigned claimed;
    const int Rpad = a.passes * kDbLanesPassRows;
    const int stride = Rpad + 4;  // = 4 (mod 8) dwords: rows of different letters start on different banks
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = lane & (G - 1), grp = lane / G;
    const int slot = (blockIdx.x * kDbLanesWaves + wave) * kDbLanesSubj + grp;
    const int go = a.go, ge = a.ge;
    const int go4 = 4 * go, ge4 = 4 * ge;
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
        const DbaUnit un = a.units[u];
        const DbaQuery qd = a.q[un.query];
        const int R = qd.R;
        if (un.query != resident)
        {
            const int* const query = a.queries + qd.off;
            for (int idx = threadIdx.x; idx < a.substsz * Rpad; idx += blockDim.x)
            {
                const int d = idx / Rpad, i = idx - d * Rpad;
                // rows past the query: below the result row, never read by it, kept out of column C's fold
                tab[d * stride + i] = i < R ? 4 * a.subst[query[i + 1] * a.substsz + d] + (int)kDbTraceDiag : kNegQ;
            }
            if (threadIdx.x == 0) atomicAdd(a.builds, 1u);
            resident = un.query;
            __syncthreads();
        }
        // the lane and register row of the result row R (in the last sweep)
        const int gR = ((R - 1) % kDbLanesPassRows) / KQ, kR = (R - 1) % KQ;
        const int tEnd = un.firstTask + un.ntasks;

        for (int t = un.firstTask + wave; t < tEnd; t += kDbLanesWaves)
        {
            const DbaTask task = a.tasks[t];
            const int s = task.first + grp;
            const bool have = grp < task.n;
            const int C = have ? a.len[s] : 0;
            const int* const x = a.db + (have ? a.off[s] : 0ll);
            // this lane's codes of column j of sweep p: cw + (p (C + 1) + j) 192
            unsigned char* const cw = a.codes + (have ? a.codeOff[s] : 0ll) + g * kDbTraceLaneBytes;
            const int Cmax = max(max(__builtin_amdgcn_readlane(C, 0), __builtin_amdgcn_readlane(C, 16)),
                                 max(__builtin_amdgcn_readlane(C, 32), __builtin_amdgcn_readlane(C, 48)));
            int result = 0;
            int colBest = cell_key4(0, kDbLanesMaxC);  // H(0, C) = 0

            for (int p = 0; p < a.passes; ++p)
            {
                const int i0 = p * kDbLanesPassRows + g * KQ;  // this lane's rows: i0 + 1 .. i0 + KQ
                const int nreal = R - i0;                      // those of them within the query: k < nreal
                int Hp[KQ], E[KQ];                             // 4 H (tag 0), 4 E (tag 0)
#pragma unroll
                for (int k = 0; k < KQ; ++k)
                {
                    Hp[k] = 0;  // column 0 is free: H = 0, no E
                    E[k] = kNegQ;
                }
                const bool last = p + 1 == a.passes;
                result = cell_key4(0, kDbLanesMaxC);  // column 0 of row R is a candidate
                int hdiag = 0;                        // H(i0, 0)
                int fLast = kNegQ | (int)kDbTraceF;
                const bool reads = p > 0 && g == 0, writes = p + 1 < a.passes && g == G - 1;
                // the letter and the row above of the next step, loaded one step ahead
                int letNext = (1 - g >= 1 && 1 - g <= C) ? x[1 - g] : 0;
                int2 bndNext = make_int2(0, kNegQ | (int)kDbTraceF);
                if (reads && C >= 1) bndNext = bnd[1];
                const int* const trow = tab + i0;
                unsigned char* const cp = cw + (size_t)p * (size_t)(C + 1) * kDbTraceColBytes;

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
                    if (p == 0) above = make_int2(0, kNegQ | (int)kDbTraceF);  // the free row 0
                    const int hu0 = from_lane_above(above.x, Hp[KQ - 1]);
                    const int fu0 = AFFINE ? from_lane_above(above.y, fLast) : 0;
                    if (j >= 1 && j <= C)
                    {
                        const int4* const tr = reinterpret_cast<const int4*>(trow + let * stride);
                        const int jc = kDbLanesMaxC - j;
                        int hup = hu0, fup = fu0, hdg = hdiag;
                        unsigned acc[KQ / 8];
#pragma unroll
                        for (int w = 0; w < KQ / 8; ++w) acc[w] = 0u;
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
                                const int d = hdg + sk[r];  // tag 2
                                int e, f, h;
                                unsigned nib;
                                if (AFFINE)
                                {
                                    const int eq = max(E[k] + ge4, hp + (go4 + 1));  // bit 0: opened
                                    const int fq = max(fup + ge4, hup + (go4 + 2));  // bit 1: opened
                                    e = eq & ~3;                                     // tag 0
                                    f = (fq & ~3) | (int)kDbTraceF;                  // tag 1
                                    nib = ((unsigned)eq & 1u) | ((unsigned)fq & 2u);
                                    E[k] = e;
                                    fup = f;
                                }
                                else
                                {
                                    e = hp + go4;
                                    f = hup + (go4 + (int)kDbTraceF);
                                    nib = 0u;
                                }
                                h = max(max(d, e), f);
                                nib = (nib << 2) | ((unsigned)h & 3u);
                                acc[k / 8] |= nib << (4 * (k % 8));
                                h &= ~3;
                                hdg = hp;
                                Hp[k] = h;
                                hup = h;
                            }
                            // Four rows' codes are formed before the chain goes on (an empty statement that
                            // ties H of the last row to the codes' dword): else the compiler runs the chain
                            // through all 24 rows first and keeps every row's values for its code.
                            asm volatile("" : "+v"(hup), "+v"(acc[(4 * q + 3) / 8]));
                        }
                        fLast = fup;
                        hdiag = hu0;
                        if (writes) bnd[j] = make_int2(hup, fup);
                        // "opened" to "extended"
                        const unsigned flip = AFFINE ? 0xccccccccu : 0u;
                        *reinterpret_cast<Codes3*>(cp + (size_t)j * kDbTraceColBytes) =
                            Codes3 {acc[0] ^ flip, acc[1] ^ flip, acc[2] ^ flip};
                        if (last)
                        {
                            // Hp[kR] by the bits of kR: five masks, not one per row; lane gR's is row R
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
                            result = max(result, cell_key4(v[0], jc));
                        }
                    }
                }
                if (nreal > 0)
                {
                    // Column C, once per lane and sweep: a lane's rows are not touched after its step C + g, so
                    // behind the loop Hp is column C in every lane (no hit: column 0).  Its rows i <= R only.
                    int m = kNoKey;
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        m = max(m, k < nreal ? (int)(((unsigned)Hp[k] << (kStepBits - 2)) | (unsigned)(KQ - 1 - k)) : kNoKey);
                    const int k = KQ - 1 - (m & ((1 << kStepBits) - 1));
                    colBest = max(colBest, cell_key4((m >> kStepBits) * 4, kDbLanesMaxC - (i0 + k + 1)));
                }
                // the next sweep's lane 0 reads what this sweep's lane 15 wrote
                if (p + 1 < a.passes) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            }
            // column C over the hit's 16 lanes: every lane gets the best key
            colBest = max(colBest, row_rotated<8>(colBest));
            colBest = max(colBest, row_rotated<4>(colBest));
            colBest = max(colBest, row_rotated<2>(colBest));
            colBest = max(colBest, row_rotated<1>(colBest));
            if (have && g == gR)
            {
                const int rowV = result >> kDbLanesJBits, colV = colBest >> kDbLanesJBits;
                a.out[s] = rowV >= colV ? DbLanesOut {rowV, R, kDbLanesMaxC - (result & kDbLanesMaxC), 0}
                                        : DbLanesOut {colV, kDbLanesMaxC - (colBest & kDbLanesMaxC), C, 0};
            }
        }
    }
}

// One lane per hit.  State kWalkH, or kDbTraceF / kDbTraceE inside a gap; every trip of the loop
// emits one move or ends the walk, so a hit takes at most R + C trips.
__global__ __launch_bounds__(kWalkThreads) void nw_dboverlap_walk_kernel(DbTraceMultiWalkArgs a)
{
    const int h = blockIdx.x * kWalkThreads + threadIdx.x;
    if (h >= a.nhits) return;
    const DbLanesOut o = a.out[h];
    const int C = a.len[h];
    const int* const x = a.db + a.off[h];
    const int* const y = a.queries + a.qoff[h];
    const unsigned char* const cb = a.codes + a.codeOff[h];
    unsigned char* const mv = a.moves + a.moveOff[h];
    int i = o.i_end, j = o.j_end, n = 0;
    unsigned state = kWalkH;
    // both borders are free: the walk ends as soon as it stands on row 0 or on column 0
    while (i > 0 && j > 0)
    {
        const int r = i - 1;
        const int p = r / kDbLanesPassRows, rr = r - p * kDbLanesPassRows;
        const int g = rr / KQ, k = rr - g * KQ;
        const size_t at = ((size_t)p * (size_t)(C + 1) + (size_t)j) * kDbTraceColBytes +
                          (size_t)(g * kDbTraceLaneBytes + (k >> 3) * 4);
        const unsigned code = (*reinterpret_cast<const unsigned*>(cb + at) >> (4 * (k & 7))) & 15u;
        const unsigned eff = state == kWalkH ? (code & 3u) : state;
        const bool diag = eff == kDbTraceDiag, up = eff == kDbTraceF, left = eff == kDbTraceE;
        if (!(diag || up || left)) break;  // no cell inside the borders has another source
        const bool ext = (up && (code & kDbTraceFExt)) || (left && (code & kDbTraceEExt));
        const bool same = y[i] == x[j];
        mv[n++] = diag ? (same ? '=' : 'X') : (up ? 'I' : 'D');
        i -= (diag || up) ? 1 : 0;
        j -= (diag || left) ? 1 : 0;
        state = ext ? eff : kWalkH;
    }
    DbTraceOut res;
    res.score = o.score;
    res.i_end = o.i_end;
    res.j_end = o.j_end;
    res.i_start = i;
    res.j_start = j;
    res.moves = n;
    res.pad0 = res.pad1 = 0;
    a.res[h] = res;
}

template <bool AFFINE>
hipError_t prepare(size_t lds, int* wgs)
{
    auto kern = nw_dboverlap_fill_kernel<AFFINE>;
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
hipError_t launch(const DbTraceMultiArgs& a, int grid, hipStream_t st)
{
    auto kern = nw_dboverlap_fill_kernel<AFFINE>;
    const size_t lds = dblanes_lds_bytes(a.passes * kDbLanesPassRows, a.substsz);
    hipError_t e = record_foot((const void*)kern, lds, 64 * kDbLanesWaves, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kDbLanesWaves), lds, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t dboverlap_trace_resident(int passes, int substsz, bool affine, int* wgs)
{
    const size_t lds = dblanes_lds_bytes(passes * kDbLanesPassRows, substsz);
    return affine ? prepare<true>(lds, wgs) : prepare<false>(lds, wgs);
}

hipError_t launch_dboverlap_trace_fill(const DbTraceMultiArgs& a, int grid, hipStream_t st)
{
    return a.go != a.ge ? launch<true>(a, grid, st) : launch<false>(a, grid, st);
}

hipError_t launch_dboverlap_trace_walk(const DbTraceMultiWalkArgs& a, hipStream_t st)
{
    if (a.nhits <= 0) return hipSuccess;
    hipLaunchKernelGGL(nw_dboverlap_walk_kernel, dim3((a.nhits + kWalkThreads - 1) / kWalkThreads), dim3(kWalkThreads),
                       0, st, a);
    return hipGetLastError();
}

}  // namespace gsa
