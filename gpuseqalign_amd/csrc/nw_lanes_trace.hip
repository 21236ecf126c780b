// nw_lanes_trace.hip -- database search, the alignments of chosen hits (gsa_align_db_dev; DESIGN.md
// 2.2e): NW / SW with linear or affine gaps, traced on the device.
//
// The fill is the lane kernel of nw_lanes.hip with one addition: a hit sits on the 16 lanes of a DPP
// row, a lane holds kDbLanesKQ = 24 query rows and walks the columns one behind the lane above
// (row_shr:1), lanes outside their hit's columns are masked by EXEC, the query profile is in LDS and a
// query of more than 384 rows takes several sweeps over the per-wave boundary array.  Per cell it
// forms a 4-bit code -- the source of H (E, F, diagonal, stop), "E was extended", "F was extended" --
// and ORs it into three dwords; a lane stores its 24 codes of a column with one 12-byte store at
//   codes[hit] + ((sweep (C + 1) + j) 16 + g) 12,
// so the 16 lanes of a hit write 192 contiguous bytes per column.  The linear instances write the
// same format with the extend bits zero.  The local instances keep the score kernel's row-best keys
// and so find the same end cell.  No wave waits for another; there are no spin loops.
//
// The walk takes one lane per hit: from (i_end, j_end) in state H it reads one nibble per move and
// selects the next state with compares ("tie rule"), writes one byte per move, last
// move first, and the cell the path starts at.  The codes never leave the device.
#include "nw_lanes_trace.h"

#include <algorithm>

#include "nw_strip.h"

namespace gsa {

namespace {

constexpr int G = kDbLanesG;
constexpr int KQ = kDbLanesKQ;
constexpr int kNegQ = -(1 << 29);  // 4 x "minus infinity" (-2^27), tag 0
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

// Values are kept as q = 4 v + tag.  The tag orders equal values the way the tie rule does, so that
// one maximum picks the value and its source at once: H = max3(diagonal | 2, F | 1, E | 0) [, 3 if
// local: H = 0 stops], and the two low bits of the maximum are the cell's source code.  E and F take
// their own candidates as (extend | 0, open | 1) and (extend | 1, open | 2): opening wins a tie, and
// bit 0 of E, bit 1 of F say "opened" -- the codes' extend bits are their complement, flipped once
// per dword.  The table in LDS holds 4 s + 2.  gsa_align_db_dev sends only pairs whose values stay
// within kDbTraceMaxValue here, so that 4 v does not leave int32.
template <bool LOCAL, bool AFFINE>
__global__ __launch_bounds__(64 * kDbLanesWaves) void nw_dbtrace_fill_kernel(DbLanesArgs a, unsigned char* codes,
                                                                             const long long* codeOff)
{
    extern __shared__ __attribute__((aligned(16))) int tab[];
    const int Rpad = a.passes * kDbLanesPassRows;
    const int stride = Rpad + 4;  // = 4 (mod 8) dwords: rows of different letters start on different banks
    for (int idx = threadIdx.x; idx < a.substsz * Rpad; idx += blockDim.x)
    {
        const int d = idx / Rpad, i = idx - d * Rpad;
        // rows past the query: never the result row, and with NEG never above a real cell (local)
        tab[d * stride + i] = i < a.R ? 4 * a.subst[a.query[i + 1] * a.substsz + d] + (int)kDbTraceDiag : kNegQ;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int g = lane & (G - 1), grp = lane / G;
    const int slot = (blockIdx.x * kDbLanesWaves + (threadIdx.x >> 6)) * kDbLanesSubj + grp;
    const int go = a.go, ge = a.ge;
    const int go4 = 4 * go, ge4 = 4 * ge;
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
        // this lane's codes of column j of sweep p: cw + (p (C + 1) + j) 192
        unsigned char* const cw = codes + (have ? codeOff[s] : 0ll) + g * kDbTraceLaneBytes;
        const int Cmax = max(max(__builtin_amdgcn_readlane(C, 0), __builtin_amdgcn_readlane(C, 16)),
                             max(__builtin_amdgcn_readlane(C, 32), __builtin_amdgcn_readlane(C, 48)));
        int bestS = 0, bi = 0, bj = 0, result = 0;

        for (int p = 0; p < a.passes; ++p)
        {
            const int i0 = p * kDbLanesPassRows + g * KQ;  // this lane's rows: i0 + 1 .. i0 + KQ
            int Hp[KQ], E[KQ], rb[KQ];                     // 4 H (tag 0), 4 E (tag 0), the row's best key
#pragma unroll
            for (int k = 0; k < KQ; ++k)
            {
                Hp[k] = LOCAL ? 0 : go4 + (i0 + k) * ge4;  // column 0
                E[k] = kNegQ;
                rb[k] = 0;
            }
            int hdiag = (LOCAL || i0 == 0) ? 0 : go4 + (i0 - 1) * ge4;  // H(i0, 0)
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
                if (p == 0)
                {
                    above.x = LOCAL ? 0 : go4 + (j - 1) * ge4;  // the border row
                    above.y = kNegQ | (int)kDbTraceF;
                }
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
                                const int eq = max(E[k] + ge4, hp + (go4 + 1));       // bit 0: opened
                                const int fq = max(fup + ge4, hup + (go4 + 2));       // bit 1: opened
                                e = eq & ~3;                                          // tag 0
                                f = (fq & ~3) | (int)kDbTraceF;                       // tag 1
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
                            if (LOCAL) h = max(h, (int)kDbTraceStop);
                            nib = (nib << 2) | ((unsigned)h & 3u);
                            acc[k / 8] |= nib << (4 * (k % 8));
                            h &= ~3;
                            hdg = hp;
                            Hp[k] = h;
                            hup = h;
                            if (LOCAL) rb[k] = max(rb[k], (int)(((unsigned)h << (kDbLanesJBits - 2)) | (unsigned)jc));
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
                    if (k == kR) result = Hp[k] >> 2;
            }
            // the next sweep's lane 0 reads what this sweep's lane 15 wrote
            if (p + 1 < a.passes) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        }
        if (LOCAL)
        {
            // the 16 lanes of a hit hold disjoint rows: the best score, then the smallest row
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

// One lane per hit.  State kWalkH, or kDbTraceF / kDbTraceE inside a gap; every trip of the loop
// emits one move or ends the walk, so a hit takes at most R + C trips.
__global__ __launch_bounds__(kWalkThreads) void nw_dbtrace_walk_kernel(DbTraceArgs a)
{
    const int h = blockIdx.x * kWalkThreads + threadIdx.x;
    if (h >= a.fill.nsubj) return;
    const DbLanesOut o = a.fill.out[h];
    const int C = a.fill.len[h];
    const int* const x = a.fill.db + a.fill.off[h];
    const int* const y = a.fill.query;
    const unsigned char* const cb = a.codes + a.codeOff[h];
    unsigned char* const mv = a.moves + a.moveOff[h];
    const bool local = a.local != 0;
    int i = o.i_end, j = o.j_end, n = 0;
    unsigned state = kWalkH;
    bool done = local && o.score == 0;
    while (!done)
    {
        const bool border = i == 0 || j == 0;
        unsigned code = 0u;
        if (!border)
        {
            const int r = i - 1;
            const int p = r / kDbLanesPassRows, rr = r - p * kDbLanesPassRows;
            const int g = rr / KQ, k = rr - g * KQ;
            const size_t at = ((size_t)p * (size_t)(C + 1) + (size_t)j) * kDbTraceColBytes +
                              (size_t)(g * kDbTraceLaneBytes + (k >> 3) * 4);
            code = (*reinterpret_cast<const unsigned*>(cb + at) >> (4 * (k & 7))) & 15u;
        }
        // on the border: local H is 0 there (stop); global row 0 is E only, column 0 F only
        const unsigned bsrc = local ? kDbTraceStop : (i == 0 ? (j == 0 ? kDbTraceStop : kDbTraceE) : kDbTraceF);
        const unsigned src = border ? bsrc : (code & 3u);
        const unsigned eff = (state == kWalkH || border) ? src : state;
        const bool diag = eff == kDbTraceDiag, up = eff == kDbTraceF, left = eff == kDbTraceE;
        done = eff == kDbTraceStop;
        const bool ext = !border && ((up && (code & kDbTraceFExt)) || (left && (code & kDbTraceEExt)));
        const bool same = y[max(i, 1)] == x[max(j, 1)];
        const unsigned char op = diag ? (same ? '=' : 'X') : (up ? 'I' : 'D');
        if (!done) mv[n] = op;
        n += done ? 0 : 1;
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

template <bool LOCAL, bool AFFINE>
hipError_t prepare(size_t lds, int* wgs)
{
    auto kern = nw_dbtrace_fill_kernel<LOCAL, AFFINE>;
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
hipError_t launch_fill(const DbTraceArgs& a, int grid, hipStream_t st)
{
    auto kern = nw_dbtrace_fill_kernel<LOCAL, AFFINE>;
    const size_t lds = dblanes_lds_bytes(a.fill.R, a.fill.substsz);
    hipError_t e = record_foot((const void*)kern, lds, 64 * kDbLanesWaves, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kDbLanesWaves), lds, st, a.fill, a.codes, a.codeOff);
    return hipGetLastError();
}

}  // namespace

hipError_t dbtrace_resident(int R, int substsz, int local, bool affine, int* wgs)
{
    const size_t lds = dblanes_lds_bytes(R, substsz);
    if (local) return affine ? prepare<true, true>(lds, wgs) : prepare<true, false>(lds, wgs);
    return affine ? prepare<false, true>(lds, wgs) : prepare<false, false>(lds, wgs);
}

hipError_t launch_dbtrace(const DbTraceArgs& a, int grid, hipEvent_t* ev, hipStream_t st)
{
    const bool affine = a.fill.go != a.fill.ge;
    if (ev) (void)hipEventRecord(ev[0], st);
    hipError_t e;
    if (a.local)
        e = affine ? launch_fill<true, true>(a, grid, st) : launch_fill<true, false>(a, grid, st);
    else
        e = affine ? launch_fill<false, true>(a, grid, st) : launch_fill<false, false>(a, grid, st);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(nw_dbtrace_walk_kernel, dim3((a.fill.nsubj + kWalkThreads - 1) / kWalkThreads),
                       dim3(kWalkThreads), 0, st, a);
    e = hipGetLastError();
    if (ev) (void)hipEventRecord(ev[2], st);
    return e;
}

}  // namespace gsa
