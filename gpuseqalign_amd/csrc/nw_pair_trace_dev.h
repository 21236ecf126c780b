// nw_pair_trace_dev.h -- the device code and the launch glue the six long-pair trace units share
// (DESIGN.md 2.2i - 2.2n): the table load, the fill of one strip by one wave, the one-lane walks of the
// three shapes, and the grid sizing and launch of a fill kernel.  Included by nw_pair_trace.hip,
// nw_pair_semi_trace.hip, nw_pair_overlap_trace.hip and their _batch units, whose kernels decode a task
// (from their arguments and the ticket, or from a descriptor table) and name a border policy.
//
// The K-rows score kernel leaves the bottom row of every ticket but the last in its hand-off granules
// (Hgo' and, affine, F', shifted; nw_krow.hip ks_drain).  With those rows exact, the strip of rows
// t TR + 1 ... (t + 1) TR depends on its checkpoint row and on the column left of its first one only, so
// all strips of a chunk are filled at once, each by one wave, and no wave waits for another: no hand-off,
// no progress words, no spin loops.  Lane l of a strip's wave holds the rows l KR + 1 ... (l + 1) KR of
// the strip (KR = TR / 64) and runs one column behind lane l - 1, whose last row it takes with a
// wave-wide shift by one lane (DPP wave_shr:1); lane 0 reads the checkpoint row, one column ahead, and
// unshifts it as bidi_combine_kernel does.  A strip's chain is W + 63 steps.  Lanes outside their own
// columns are masked by EXEC.  Per cell the fill forms the 4-bit code of nw_lanes_trace.hip with the same
// tagged maximum (values kept as 4 v + tag); a lane's codes of a column are KR / 2 bytes, a strip's
// column 32 KR contiguous bytes.  The substitution values come from a copy of the table in LDS
// (4 s + 2, transposed), gathered by the lane's own row letters.
//
// The strip fill sets every piece of per-task state (yo, Hp, E, hdiag, fLast, letNext, aboveNext) anew when
// it is entered: a workgroup may run it for strips of different pairs back to back.  It holds no atomic,
// no barrier and no unbounded loop: its loops are bounded by W + 63 and KR; the ticket loop is the
// calling kernel's.
//
// A walk takes one lane: a nibble load and a move per trip, across strip boundaries by address
// arithmetic, until the path's first cell or the chunk's upper boundary, where it leaves the cell and
// its state for the next chunk.  Every trip emits one move or ends the walk.
//
// Why the strip fill, the walk loops and the walk's step are statement macros and not __forceinline__
// templates like the rest: the compiler optimises a function's body once on its own and again after it
// is inlined, and that second round alone changes the code of every kernel here (fewer VGPRs in the
// affine fills, more SGPRs in the walks), whatever the function's signature.  The tests pin all 38 kernels
// to the registers, occupancy and LDS they had with the body written out in each kernel, so the body
// stands in the kernel's own text and is optimised once, as before.  The macros are used inside
// `using namespace pair_dev` and declare their locals in a block of their own, where they hide the
// caller's variables of the same name: GSA_PAIR_STRIP_FILL declares lane, s, x, W, jW, J, c, step, k, w
// (and TR, NW, go4, ge4, iT, i0, ck, gh, gf, cw, yo, Hp, E, hdiag, fLast, letNext, aboveNext), the walk
// macros r, o, i, j, n, state, done, left, jW, border, code, bsrc, src.  So no argument may be an
// expression over one of those names; `task`, `w` and `rec` are lvalues, `tab`, `ssz`, `go`, `ge` and
// `local` plain values that are read at every use, and BORDER, AFFINE, KR and STOPS constant expressions
// (a compound one in parentheses).  A walk macro needs its shape's record type (PairWalkRec, SemiWalkRec,
// OverlapWalkRec) only where it is expanded: the unit's own header declares it.
#pragma once
#include <algorithm>

#include "nw_lanes_trace.h"
#include "nw_strip.h"

namespace gsa {
namespace pair_dev {

constexpr int kNegQ = -(1 << 29);  // 4 x "minus infinity" (-2^27), tag 0
constexpr unsigned kWalkH = 4u;    // the walk's state H; inside a gap the state is the gap's source code
constexpr int kFillWgsPerCu = 8;

__device__ __forceinline__ int from_lane_above(int own, int src)
{
    // wave_shr:1 over the 64 lanes; lane 0 has no source and keeps `own`
    return __builtin_amdgcn_update_dpp(own, src, 0x138, 0xf, 0xf, false);
}

template <int N>
struct __attribute__((aligned(4 * N))) CodesN
{
    unsigned w[N];
};

// The checkpoint row above strip s at column j, as 4 H (tag 0) and 4 F | F's tag: the low 32 bits of
// the granule, signed, H = Hgo' - (go - ge) + (i + j) ge, F = F' + (i + j) ge.  Local: the score
// kernel's F' has the zero floor folded in, so F here is max(F, 0); a walk is in state F only at
// cells with F = H > 0, and the floor adds at most 0 + ge <= 0 to the row below, never the winner.
template <bool AFFINE>
__device__ __forceinline__ int2 checkpoint(const unsigned long long* gh, const unsigned long long* gf, int j, int iT,
                                           int go, int ge)
{
    const int sh = (iT + j) * ge;
    const int h = (int)(unsigned)gh[j] - (go - ge) + sh;
    int2 r;
    r.x = 4 * h;
    r.y = AFFINE ? ((4 * ((int)(unsigned)gf[j] + sh)) | (int)kDbTraceF) : 0;
    return r;
}

// tab[x letter][y letter] = 4 s(y, x) + tag "diagonal", by the 64 threads of the workgroup; the caller
// puts a barrier behind it
__device__ __forceinline__ void load_tab(int* tab, const int* subst, int ssz)
{
    for (int idx = threadIdx.x; idx < ssz * ssz; idx += 64)
    {
        const int xl = idx / ssz, yl = idx - xl * ssz;
        tab[idx] = 4 * subst[yl * ssz + xl] + (int)kDbTraceDiag;
    }
}

// What stands around a strip's cells:
//   kGlobal   row 0 and column 0 are gap runs from (0, 0);
//   kLocal    row 0 and column 0 are 0, and every H has the floor 0 (code kDbTraceStop);
//   kSemi     row 0 is free (H = 0, F = minus infinity); the column left of the window is the global
//             column 0 if jW = 0, minus infinity below row 0 otherwise;
//   kOverlap  row 0 and column 0 are free: H = 0, no gap runs along either.
enum Border
{
    kGlobal,
    kLocal,
    kSemi,
    kOverlap
};

// One strip of one pair, as its kernel decoded it.  Columns count within the window: window column c is
// the pair's column jW + c (jW = 0 but for kSemi), and x, gh and gf are offset by jW already.
struct StripTask
{
    int s;              // the strip: rows s TR + 1 ... (s + 1) TR
    const int* seqY;    // rows, letters at 1 ...
    const int* x;       // x[c]: the letter of window column c
    int clampRow;       // rows past it take its letter
    int lastRow;        // lanes whose rows all lie below it have no cells
    int W;              // window columns 1 ... W
    int jW;             // the window's left column (kSemi)
    const unsigned long long* gh;  // the checkpoint row above the strip (s > 0): Hgo' at [c]
    const unsigned long long* gf;  // F' (affine)
    unsigned char* cw;  // the strip's codes: window column c at (c - 1) TR / 2, lane l at l KR / 2
};

// The fill of one strip by the 64 lanes of its wave: `task` is a StripTask, `tab` the table in LDS
// (load_tab), ssz its side, go and ge the gap scores.
#define GSA_PAIR_STRIP_FILL(BORDER, AFFINE, KR, task, tab, ssz, go, ge)                                              \
    do                                                                                                               \
    {                                                                                                                \
        constexpr int TR = 64 * KR;                                                                                  \
        constexpr int NW = KR / 8; /* dwords of codes per lane and column */                                         \
        const int lane = threadIdx.x;                                                                                \
        const int go4 = 4 * (go), ge4 = 4 * (ge);                                                                    \
        const int* const x = (task).x;                                                                               \
        const int s = (task).s, W = (task).W, jW = (task).jW;                                                        \
        const int iT = s * TR; /* the checkpoint row (0: the border) */                                              \
        const int i0 = iT + lane * KR; /* this lane's rows: i0 + 1 ... i0 + KR */                                    \
        const int J = i0 < (task).lastRow ? W : 0;                                                                   \
        const bool ck = s > 0 && lane == 0;                                                                          \
        const unsigned long long* const gh = (task).gh;                                                              \
        const unsigned long long* const gf = (task).gf;                                                              \
        unsigned char* const cw = (task).cw + lane * (KR / 2);                                                       \
        int yo[KR], Hp[KR], E[KR]; /* the rows' letters, 4 H (tag 0), 4 E (tag 0) */                                 \
        _Pragma("unroll") for (int k = 0; k < KR; ++k)                                                               \
        {                                                                                                            \
            yo[k] = (task).seqY[min(i0 + 1 + k, (task).clampRow)];                                                   \
            /* the column left of the window */                                                                      \
            if (BORDER == kGlobal) Hp[k] = go4 + (i0 + k) * ge4;                                                     \
            else if (BORDER == kSemi) Hp[k] = jW > 0 ? kNegQ : go4 + (i0 + k) * ge4;                                 \
            else Hp[k] = 0;                                                                                          \
            E[k] = kNegQ;                                                                                            \
        }                                                                                                            \
        int hdiag; /* H(i0, left column) */                                                                          \
        if (BORDER == kGlobal) hdiag = i0 == 0 ? 0 : go4 + (i0 - 1) * ge4;                                           \
        else if (BORDER == kSemi) hdiag = i0 == 0 ? 0 : (jW > 0 ? kNegQ : go4 + (i0 - 1) * ge4);                     \
        else hdiag = 0;                                                                                              \
        int fLast = kNegQ | (int)kDbTraceF;                                                                          \
        /* the letter and the row above of the next step, loaded one step ahead */                                   \
        int letNext = (1 - lane >= 1 && 1 - lane <= J) ? x[1 - lane] : 0;                                            \
        int2 aboveNext = make_int2(0, kNegQ | (int)kDbTraceF);                                                       \
        if (ck && J >= 1) aboveNext = checkpoint<AFFINE>(gh, gf, 1, iT, (go), (ge));                                 \
        for (int step = 1; step <= W + 63; ++step)                                                                   \
        {                                                                                                            \
            const int c = step - lane;                                                                               \
            const int let = letNext;                                                                                 \
            int2 above = aboveNext;                                                                                  \
            if (c + 1 >= 1 && c + 1 <= J)                                                                            \
            {                                                                                                        \
                letNext = x[c + 1];                                                                                  \
                if (ck) aboveNext = checkpoint<AFFINE>(gh, gf, c + 1, iT, (go), (ge));                               \
            }                                                                                                        \
            if (s == 0)                                                                                              \
            {                                                                                                        \
                above.x = BORDER == kGlobal ? go4 + (c - 1) * ge4 : 0; /* the border row: E only, or free */         \
                above.y = kNegQ | (int)kDbTraceF;                                                                    \
            }                                                                                                        \
            const int hu0 = from_lane_above(above.x, Hp[KR - 1]);                                                    \
            const int fu0 = AFFINE ? from_lane_above(above.y, fLast) : 0;                                            \
            if (c >= 1 && c <= J)                                                                                    \
            {                                                                                                        \
                const int* const trow = (tab) + let * (ssz);                                                         \
                int hup = hu0, fup = fu0, hdg = hdiag;                                                               \
                unsigned acc[NW];                                                                                    \
                _Pragma("unroll") for (int w = 0; w < NW; ++w) acc[w] = 0u;                                          \
                _Pragma("unroll") for (int k = 0; k < KR; ++k)                                                       \
                {                                                                                                    \
                    const int hp = Hp[k];                                                                            \
                    const int d = hdg + trow[yo[k]]; /* tag 2 */                                                     \
                    int e, f, h;                                                                                     \
                    unsigned nib;                                                                                    \
                    if (AFFINE)                                                                                      \
                    {                                                                                                \
                        const int eq = max(E[k] + ge4, hp + (go4 + 1)); /* bit 0: opened */                          \
                        const int fq = max(fup + ge4, hup + (go4 + 2)); /* bit 1: opened */                          \
                        e = eq & ~3; /* tag 0 */                                                                     \
                        f = (fq & ~3) | (int)kDbTraceF; /* tag 1 */                                                  \
                        nib = ((unsigned)eq & 1u) | ((unsigned)fq & 2u);                                             \
                        E[k] = e;                                                                                    \
                        fup = f;                                                                                     \
                    }                                                                                                \
                    else                                                                                             \
                    {                                                                                                \
                        e = hp + go4;                                                                                \
                        f = hup + (go4 + (int)kDbTraceF);                                                            \
                        nib = 0u;                                                                                    \
                    }                                                                                                \
                    h = max(max(d, e), f);                                                                           \
                    if (BORDER == kLocal) h = max(h, (int)kDbTraceStop);                                             \
                    nib = (nib << 2) | ((unsigned)h & 3u);                                                           \
                    acc[k / 8] |= nib << (4 * (k % 8));                                                              \
                    h &= ~3;                                                                                         \
                    hdg = hp;                                                                                        \
                    Hp[k] = h;                                                                                       \
                    hup = h;                                                                                         \
                }                                                                                                    \
                fLast = fup;                                                                                         \
                hdiag = hu0;                                                                                         \
                /* "opened" to "extended" */                                                                         \
                const unsigned flip = AFFINE ? 0xccccccccu : 0u;                                                     \
                CodesN<NW> out;                                                                                      \
                _Pragma("unroll") for (int w = 0; w < NW; ++w) out.w[w] = acc[w] ^ flip;                             \
                *reinterpret_cast<CodesN<NW>*>(cw + (size_t)(c - 1) * (TR / 2)) = out;                               \
            }                                                                                                        \
        }                                                                                                            \
    } while (0)

// One pair's chunk of codes and its move buffer, as the walk kernel decoded them.
struct WalkTask
{
    const int* seqY;
    const int* seqX;
    const unsigned char* codes;  // strip s at (s - tLo) stripBytes, column j at (j - jW - 1) TR / 2
    long long stripBytes;
    int krShift;  // log2 KR: 3 or 4
    int tLo;      // the chunk's first strip
    int iStop;    // stop on this row (> 0) at a column > 0: the chunk's upper boundary
    int jW;       // the window's left column (semi-global; 0 otherwise)
    unsigned char* moves;  // one byte per move, last move first
};

// The code of cell (i, j), i >= 1, j > jW: strip, lane, row in the lane, nibble
__device__ __forceinline__ unsigned walk_code(const WalkTask& w, int i, int j)
{
    const int ks = w.krShift, KR = 1 << ks, TRm = (64 << ks) - 1;
    const int rr = (i - 1) & TRm, t = ((i - 1) >> (6 + ks)) - w.tLo;
    const int l = rr >> ks, k = rr & (KR - 1);
    const size_t at = (size_t)t * (size_t)w.stripBytes + (size_t)(j - w.jW - 1) * (size_t)(32 << ks) +
                      (size_t)(l * (KR / 2) + (k >> 3) * 4);
    return (*reinterpret_cast<const unsigned*>(w.codes + at) >> (4 * (k & 7))) & 15u;
}

// One step from cell (i, j) in `state`, whose source is `src` and whose code is `code` (on a border: the
// border's source, code 0): the effective source, whether the gap it takes is an extended one, the move's
// byte ('=' or 'X' by the letters y[iy] and x[jx]) at moves[n], the cell the move leads to, and the next
// state.  STOPS: the source may be kDbTraceStop, which sets `done` and emits no move.
#define GSA_PAIR_WALK_STEP(STOPS, w, i, j, n, state, done, src, border, code, iy, jx)                                \
    do                                                                                                               \
    {                                                                                                                \
        const unsigned eff = (state == kWalkH || (border)) ? (src) : state;                                          \
        const bool diag = eff == kDbTraceDiag, up = eff == kDbTraceF, left_ = eff == kDbTraceE;                      \
        if (STOPS) done = eff == kDbTraceStop;                                                                       \
        const bool ext = !(border) && ((up && ((code) & kDbTraceFExt)) || (left_ && ((code) & kDbTraceEExt)));       \
        const bool same = (w).seqY[iy] == (w).seqX[jx];                                                              \
        const unsigned char op = diag ? (same ? '=' : 'X') : (up ? 'I' : 'D');                                       \
        if (!(STOPS) || !done) (w).moves[n] = op;                                                                    \
        n += ((STOPS) && done) ? 0 : 1;                                                                              \
        i -= (diag || up) ? 1 : 0;                                                                                   \
        j -= (diag || left_) ? 1 : 0;                                                                                \
        state = ext ? eff : kWalkH;                                                                                  \
    } while (0)

// Global or local: to (0, 0), or to the first cell whose code is kDbTraceStop.  w: a WalkTask; rec: the
// pair's PairWalkRec in device memory, read at the start and written at the end.
#define GSA_PAIR_WALK(w, local, rec)                                                                                 \
    do                                                                                                               \
    {                                                                                                                \
        const PairWalkRec r = (rec);                                                                                 \
        int i = r.i, j = r.j, n = r.n;                                                                               \
        unsigned state = r.state;                                                                                    \
        bool done = r.done != 0;                                                                                     \
        while (!done && !((w).iStop > 0 && i == (w).iStop && j > 0))                                                 \
        {                                                                                                            \
            const bool border = i == 0 || j == 0;                                                                    \
            unsigned code = 0u;                                                                                      \
            if (!border) code = walk_code((w), i, j);                                                                \
            /* on the border: local H is 0 there (stop); global row 0 is E only, column 0 F only */                  \
            const unsigned bsrc =                                                                                    \
                (local) ? kDbTraceStop : (i == 0 ? (j == 0 ? kDbTraceStop : kDbTraceE) : kDbTraceF);                 \
            const unsigned src = border ? bsrc : (code & 3u);                                                        \
            GSA_PAIR_WALK_STEP(true, w, i, j, n, state, done, src, border, code, max(i, 1), max(j, 1));              \
        }                                                                                                            \
        PairWalkRec o;                                                                                               \
        o.i = i;                                                                                                     \
        o.j = j;                                                                                                     \
        o.state = state;                                                                                             \
        o.n = n;                                                                                                     \
        o.done = done ? 1 : 0;                                                                                       \
        o.pad0 = o.pad1 = o.pad2 = 0;                                                                                \
        (rec) = o;                                                                                                   \
    } while (0)

// Semi-global: stops as soon as it is in row 0, takes F ('I') on column 0 below it, and flags a step onto
// column jW > 0 below row 0, which the window's bound excludes.  rec: the pair's SemiWalkRec.
#define GSA_SEMI_WALK(w, rec)                                                                                        \
    do                                                                                                               \
    {                                                                                                                \
        const SemiWalkRec r = (rec);                                                                                 \
        const int jW = (w).jW;                                                                                       \
        int i = r.i, j = r.j, n = r.n, left = r.left;                                                                \
        unsigned state = r.state;                                                                                    \
        bool done = r.done != 0;                                                                                     \
        while (!done && !((w).iStop > 0 && i == (w).iStop && j > 0))                                                 \
        {                                                                                                            \
            if (i == 0)                                                                                              \
            {                                                                                                        \
                done = true; /* in row 0: the subject's head stays out of the alignment */                           \
                break;                                                                                               \
            }                                                                                                        \
            if (j == jW && jW > 0)                                                                                   \
            {                                                                                                        \
                left = 1; /* outside the window */                                                                   \
                done = true;                                                                                         \
                break;                                                                                               \
            }                                                                                                        \
            const bool border = j == 0; /* column 0 below row 0: F only */                                           \
            unsigned code = 0u;                                                                                      \
            if (!border) code = walk_code((w), i, j);                                                                \
            const unsigned src = border ? kDbTraceF : (code & 3u);                                                   \
            GSA_PAIR_WALK_STEP(false, w, i, j, n, state, done, src, border, code, i, max(j, 1));                     \
        }                                                                                                            \
        if (i == 0) done = true;                                                                                     \
        SemiWalkRec o;                                                                                               \
        o.i = i;                                                                                                     \
        o.j = j;                                                                                                     \
        o.state = state;                                                                                             \
        o.n = n;                                                                                                     \
        o.done = done ? 1 : 0;                                                                                       \
        o.left = left;                                                                                               \
        o.pad0 = o.pad1 = 0;                                                                                         \
        (rec) = o;                                                                                                   \
    } while (0)

// Overlap: stops as soon as it stands on row 0 or on column 0 and emits no letter along either.  rec: the
// pair's OverlapWalkRec.
#define GSA_OVERLAP_WALK(w, rec)                                                                                     \
    do                                                                                                               \
    {                                                                                                                \
        const OverlapWalkRec r = (rec);                                                                              \
        int i = r.i, j = r.j, n = r.n;                                                                               \
        unsigned state = r.state;                                                                                    \
        bool done = r.done != 0;                                                                                     \
        while (!done && !((w).iStop > 0 && i == (w).iStop && j > 0))                                                 \
        {                                                                                                            \
            if (i == 0 || j == 0)                                                                                    \
            {                                                                                                        \
                done = true; /* on a free border: the overhang stays out of the alignment */                         \
                break;                                                                                               \
            }                                                                                                        \
            const unsigned code = walk_code((w), i, j);                                                              \
            GSA_PAIR_WALK_STEP(false, w, i, j, n, state, done, code & 3u, false, code, i, j);                        \
        }                                                                                                            \
        if (i == 0 || j == 0) done = true;                                                                           \
        OverlapWalkRec o;                                                                                            \
        o.i = i;                                                                                                     \
        o.j = j;                                                                                                     \
        o.state = state;                                                                                             \
        o.n = n;                                                                                                     \
        o.done = done ? 1 : 0;                                                                                       \
        o.pad0 = o.pad1 = o.pad2 = 0;                                                                                \
        (rec) = o;                                                                                                   \
    } while (0)

// The grid of a fill kernel: one workgroup per task, at most what fits on the device at kFillWgsPerCu
// per CU, and at most maxWgs if that is positive.
template <class Kernel>
hipError_t fill_grid_for(Kernel kernel, int ntasks, int maxWgs, int* grid)
{
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0);
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    int g = std::max(1, std::min(ntasks, std::min(std::max(1, per_cu), kFillWgsPerCu) * std::max(1, cus)));
    if (maxWgs > 0) g = std::min(g, maxWgs);
    *grid = g;
    return hipSuccess;
}

template <class Kernel, class Args>
hipError_t launch_fill_for(Kernel kernel, const Args& args, int grid, hipStream_t st)
{
    hipError_t e = record_foot((const void*)kernel, 0, 64, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, st, args);
    return hipGetLastError();
}

}  // namespace pair_dev
}  // namespace gsa
