/*
 * gsa.h -- C ABI of the MI355X NW-LG engine (libgsa.so).
 *
 * This is the drop-in boundary for the reference's align slot
 *     using NwAlignFn = NwStat (*)(const NwAlgParams&, NwAlgInput&, NwAlgResult&);
 * (markods/GpuSeqAlign src/nw_algorithm.hpp:11, registered in src/nw_algorithm.cpp:48-66)
 * and for the consumers the registry pairs with it (NwTrace1_Plain / NwHash1_Plain,
 * NwTrace2_Sparse / NwHash2_Sparse, src/nw_fns.hpp:22-39).  Plain pointers and sizes only.
 *
 * Conventions (identical to NwAlgInput, src/run_types.hpp:70-110):
 *  - seqY / seqX are int32 letter indices WITH the dummy header element 0
 *    (src/file_formats.cpp:43-47); adjrows = |seqY|+1, adjcols = |seqX|+1.
 *  - subst is substsz*substsz int32, row = seqY letter, column = seqX letter
 *    (src/nwalign_cpu1_st_row.cpp:6).
 *  - gapo is the linear gap cost (reference default -11, src/cmd_parser.cpp:298).
 *  - full score matrix: adjrows*adjcols int32 row-major, unpadded (nw.score).
 *  - sparse (mlsp) matrices: tileHrowMat[trows*tcols*(1+tileBx)] and
 *    tileHcolMat[trows*tcols*(1+tileBy)], tile-major row-major k = tcols*iTile + jTile
 *    (nwalign_gpu9_mlsp_diagdiagdiag.cu:15-63, :147-171, :319-358).
 *  - every int-returning function returns an NwStat code (src/run_types.hpp:12-24); the
 *    raw hipError_t of the failing runtime call is kept in the context
 *    (gsa_last_hip_error), like NwAlgResult::cudaStat.
 */
#ifndef GSA_H
#define GSA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* NwStat (src/run_types.hpp:12-24), same numbering. */
enum gsa_stat
{
    GSA_SUCCESS = 0,
    GSA_HELP_MENU_REQUESTED = 1,
    GSA_ERROR_CUDA_GENERAL = 2, /* errorCudaGeneral: HIP runtime failure */
    GSA_ERROR_MEMORY_ALLOCATION = 3,
    GSA_ERROR_MEMORY_TRANSFER = 4,
    GSA_ERROR_KERNEL_FAILURE = 5,
    GSA_ERROR_IO_STREAM = 6,
    GSA_ERROR_INVALID_FORMAT = 7,
    GSA_ERROR_INVALID_VALUE = 8,
    GSA_ERROR_INVALID_RESULT = 9
};

typedef struct gsa_ctx gsa_ctx;

/* Sparse geometry produced by a fill (NwAlgInput tileHdrMatRows/Cols, tileHrowLen/HcolLen,
 * src/run_types.hpp:97-100; set at nwalign_gpu9_mlsp_diagdiagdiag.cu:696-699). */
typedef struct gsa_sparse_geom
{
    int32_t tileBx, tileBy;
    int32_t tileHdrMatRows, tileHdrMatCols; /* trows, tcols */
    int32_t tileHrowLen, tileHcolLen;       /* 1+tileBx, 1+tileBy */
    int64_t hrowElems, hcolElems;           /* trows*tcols*(1+tileBx), trows*tcols*(1+tileBy) */
} gsa_sparse_geom;

/* Stopwatch laps of NwAlgResult::sw_align, in ms (src/stopwatch.cpp:43-50; names at
 * src/file_formats.cpp:505-519).  calc_kernel_ms is the hipEvent time of the fill kernels. */
typedef struct gsa_laps
{
    float alloc, cpy_dev, init_hdr, calc, cpy_host;
    float calc_kernel_ms;
} gsa_laps;

/* Phase-boundary callback of the host-buffer entry points (gsa_align_full, gsa_align_sparse,
 * gsa_align_sparse_pt, gsa_score): called with "align.alloc", "align.cpy_dev", "align.init_hdr",
 * "align.calc", "align.cpy_host" (and "align.calc" again after the last-tile recompute of the
 * sparse forms) at the points where the reference's align functions call Stopwatch::lap
 * (nwalign_gpu9_mlsp_diagdiagdiag.cu:435-719, nwalign_gpu3_ml_diagdiag.cu:329-593;
 * src/stopwatch.hpp:19), so an adapter drives the reference's own stopwatch:
 *     static void onLap(void* sw, const char* name) { ((Stopwatch*)sw)->lap(name); }
 *     res.sw_align.start(); gsa_set_lap_callback(ctx, onLap, &res.sw_align);
 * Called on the calling thread, before the entry point returns.  fn = NULL removes it. */
typedef void (*gsa_lap_fn)(void* user, const char* lap_name);

/* ---- context --------------------------------------------------------------------- */
/* One context per device and host thread (the reference's initNwInput, src/benchmark.cpp:175-223). */
int gsa_ctx_create(int device, gsa_ctx** out);
void gsa_ctx_destroy(gsa_ctx* ctx);
int gsa_last_hip_error(const gsa_ctx* ctx);
int gsa_device_cu_count(const gsa_ctx* ctx);
const char* gsa_version(void);
int gsa_set_lap_callback(gsa_ctx* ctx, gsa_lap_fn fn, void* user);
/* Not part of the reference's interface: the measurement / test switches, named as environment
 * variables (GSA_FULL_KERNEL, GSA_KROW_NS, ...; DESIGN.md lists them).  A context takes them from
 * the environment once, in gsa_ctx_create; this sets one for this context (value NULL: unset, the
 * built-in choice).  errorInvalidValue for a name the library does not know. */
int gsa_set_knob(gsa_ctx* ctx, const char* name, const char* value);

/* Tile height (tileBy) of the sparse representation this build produces: 1024, the rows of one
 * K-rows workgroup ticket (4 strip waves x 64 lanes x 4 rows per lane). */
int32_t gsa_sparse_tile_by(void);
/* Geometry for (adjrows, adjcols, tileBx); tileBx must be a multiple of 16 and >= 64. */
int gsa_sparse_geometry(int32_t adjrows, int32_t adjcols, int32_t tileBx, gsa_sparse_geom* geom);

/* ---- hot path, device-resident buffers (inputs already in HBM) --------------------- */
/* Enqueue the fill on `stream` (a hipStream_t; NULL = the HIP null stream); asynchronous.  Call
 * gsa_sync() before reading outputs: it also reports hand-off time-outs.  The context's error word
 * is STICKY: a time-out in any launch enqueued since the last gsa_sync() makes that gsa_sync()
 * return GSA_ERROR_KERNEL_FAILURE (launches enqueued behind the failed one give up at once), and
 * gsa_sync() then clears it, so the context is usable again.  One stream per context at a time
 * (the launches share the context's ticket word).
 * Accepted value range, the same for every fill entry point (gsa_fill_*_dev, their pitched and batch
 * forms, gsa_align_full, gsa_align_sparse, gsa_align_sparse_pt).  gapo may have any sign; substsz is
 * 1 .. 32, else errorInvalidValue before anything is enqueued.  The fill kernels keep
 * H' = H - (i + j) gapo, which is 0 on the borders and grows by q = s - 2 gapo on a diagonal step and
 * by 0 on a gap step, so 0 <= H'(i, j) <= qmax min(i, j) with qmax the largest q of the table (at
 * least 0).  With m the largest min(i, j) over the cells an output word depends on --
 *   sparse: max(min((trows - 1) tileBy, tcols tileBx), min(trows tileBy, (tcols - 1) tileBx)), the
 *           header rows' and the header columns' far corners in the padded matrix;
 *   full:   min(adjrows - 1, adjcols - 1);
 *   batch:  the largest m of its pairs --
 * a fill needs every q in [-32768, 32767] (the strip kernel, GSA_SPARSE_KERNEL=strip: [-32767, 32767])
 * and qmax m < 2^31.  The table is device memory, so the kernels test it, once per workgroup: a table
 * outside sets bit 2 of the error word before any ticket is taken, no output word is valid, and the
 * next gsa_sync() (or the host-buffer entry point itself) returns GSA_ERROR_KERNEL_FAILURE and clears
 * the word; in a batch one pair past the bound refuses the whole call.  Inside the range every word
 * is exact, on whichever instance runs (a table with some q outside [-128, 127] runs on the int16
 * instance, gsa_launch_info::q8_declined).  The one-pass lane fill (GSA_FULL_KERNEL=lane) keeps H
 * itself and takes every table whose H fits int32.  Nothing checks that H itself fits int32. */
int gsa_fill_full_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                      const int32_t* subst, int32_t substsz, int32_t gapo, int32_t* score, void* stream);
int gsa_fill_sparse_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                        const int32_t* subst, int32_t substsz, int32_t gapo, int32_t tileBx, int32_t* tileHrowMat,
                        int32_t* tileHcolMat, void* stream);
int gsa_sync(gsa_ctx* ctx, void* stream);

/* Pitched device layout of a full matrix.  The reference keeps its device score matrix padded
 * and crops it on the way back (nwalign_gpu3_ml_diagdiag.cu:315-325, cudaMemcpy2D at :585-588,
 * src/memory.hpp:217); these entry points take the row pitch `ld` (>= adjcols, in ints) of such a
 * device matrix: cell (i, j) at score[i*ld + j].  Every ld >= adjcols gives the same values.
 * gsa_full_pitch(adjcols) is the pitch this engine writes fastest: ld = 1 (mod 32), and with the
 * matrix placed gsa_full_base_offset() ints past a 128-byte boundary (cell (1, 0) on one), all
 * cells of an anti-diagonal share their offset within a 128-byte line, so the wavefront's row
 * segments are stored as whole aligned lines (no partial-line writes). */
int32_t gsa_full_pitch(int32_t adjcols);
int32_t gsa_full_base_offset(void);
int gsa_fill_full_pitched_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX,
                              int32_t adjcols, const int32_t* subst, int32_t substsz, int32_t gapo, int32_t* score,
                              int32_t ld, void* stream);
/* Peak resource use of the fills launched on this context since its creation or the last reset:
 * the reference's NwAlgResult peak-alloc columns (updateNwAlgPeakMemUsage, nwalign_shared.cpp:5-25).
 * shmem/locmem/regmem = per-workgroup LDS, per-lane scratch x threads, per-lane VGPRs x 4 B x
 * threads, each times the workgroups resident at once; glmem = device bytes the context holds
 * (scratch and hand-off buffers, plus the host-buffer entry points' input/output copies). */
typedef struct gsa_mem_stats
{
    int64_t glmem_peak_allocs, shmem_peak_allocs, locmem_peak_allocs, regmem_peak_allocs;
} gsa_mem_stats;
int gsa_mem_stats_get(const gsa_ctx* ctx, gsa_mem_stats* out);
int gsa_mem_stats_reset(gsa_ctx* ctx);
/* Hand-off watchdog: a wait inside a fill that sees no progress for this long gives up and sets
 * the error word (default 1 s; 0 = give up at the first unmet poll, for tests of the error path).
 * Applies to launches enqueued after the call. */
int gsa_set_watchdog(gsa_ctx* ctx, int64_t microseconds);

/* ---- batched fills: many independent pairs in ONE persistent launch ------------------- */
/* Device pointers of one pair: score for full fills (adjrows*adjcols), the two header
 * matrices for sparse fills (sizes from gsa_sparse_geometry). */
typedef struct gsa_pair_dev
{
    const int32_t* seqY;
    int32_t adjrows;
    const int32_t* seqX;
    int32_t adjcols;
    int32_t* score;
    int32_t* tileHrowMat;
    int32_t* tileHcolMat;
} gsa_pair_dev;
/* `pairs` is a host array of `npairs` entries; results are identical to one fill per pair.
 * The reference runs pairs one at a time through its benchmark loop (src/benchmark.cpp:
 * 393-520); a batch replaces that loop for throughput runs (BASELINE configs[3]).
 * Launches on one context must be ordered (same stream, or synchronised).  Asynchronous: a full
 * batch times its candidate schedules on its first launches with HIP events that are read only
 * once complete (never a host wait); the host blocks only when more than 4 launches' descriptors
 * are in flight on the context. */
int gsa_fill_full_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                            int32_t substsz, int32_t gapo, void* stream);
/* As gsa_fill_full_batch_dev, pair p's matrix with row pitch lds[p] (>= its adjcols; see
 * gsa_full_pitch). */
int gsa_fill_full_batch_pitched_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* lds,
                                    const int32_t* subst, int32_t substsz, int32_t gapo, void* stream);
int gsa_fill_sparse_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                              int32_t substsz, int32_t gapo, int32_t tileBx, void* stream);

/* ---- NwAlignFn equivalents, host buffers (alloc + H2D + fill + D2H, laps as the
 * reference's NwAlign_Gpu3_Ml_DiagDiag / NwAlign_Gpu9_Mlsp_DiagDiagDiag) -------------- */
int gsa_align_full(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                   const int32_t* subst, int32_t substsz, int32_t gapo, int32_t* score_out, int32_t* align_cost,
                   gsa_laps* laps);
int gsa_align_sparse(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                     const int32_t* subst, int32_t substsz, int32_t gapo, int32_t tileBx, int32_t* tileHrowMat_out,
                     int32_t* tileHcolMat_out, gsa_sparse_geom* geom, int32_t* align_cost, gsa_laps* laps);

/* mlsppt ("multi-launch sparse with parallel transfer", named in the reference's README.md:39,
 * never implemented there): as gsa_align_sparse, but the header matrices are copied back to
 * the host tile row by tile row WHILE the fill runs (the kernel flags each finished
 * super-strip in host-mapped memory).  Same outputs; the laps' cpy_host is only the tail
 * copied after the fill ends. */
int gsa_align_sparse_pt(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                        const int32_t* subst, int32_t substsz, int32_t gapo, int32_t tileBx, int32_t* tileHrowMat_out,
                        int32_t* tileHcolMat_out, gsa_sparse_geom* geom, int32_t* align_cost, gsa_laps* laps);

/* Measurement aid, not part of the reference's interface: with GSA_STAMPS=1 in the environment a
 * fused full fill records stamps: [start, end] (s_memrealtime, 100 MHz) and [start,
 * end] (s_memtime, shader clock) per pass-1 strip, then [claimed, ready, done] (s_memrealtime) per
 * expansion task; a K-rows sparse fill or a full fill's separate pass 1 records its strip ledger:
 * [realtime start, end, shader clock start, end, cycles waiting for input, waits, four block spans of
 * a diagnostic build] per strip (10 words).  Copies
 * the last such launch's *n stamps
 * into out (cap >= *n, else errorInvalidValue; out may be null to query *n); synchronizes the stream
 * that launch ran on. */
int gsa_debug_stamps(gsa_ctx* ctx, uint64_t* out, int64_t cap, int64_t* n);

/* Measurement aid, not part of the reference's interface: with timing on, every two-pass full fill
 * (gsa_fill_full*_dev) records HIP events before pass 1, between the passes and
 * after pass 2 on its stream, and pass 2's workgroups record their shader cycles (s_memtime) and
 * 100 MHz ticks (s_memrealtime) from start to end.  gsa_last_full_timing waits for the last such
 * fill and returns the pass times and the effective shader clock over pass 2's workgroups (median
 * and cycle-weighted mean), so a slow box shows as a low clock.  A fused fill (one launch) has
 * pass1_ms = -1, its whole time in pass2_ms and no clock.  A pipelined batch (groups > 0: pass 1 of
 * pair group g + 1 beside the expansion of group g) has group 0's pass 1 (alone on the chip) in
 * pass1_ms, everything after it in pass2_ms and the clock of its last expansion launch.
 * errorInvalidValue: no timed fill. */
typedef struct gsa_full_timing
{
    float pass1_ms, pass2_ms;
    float clock_ghz_median, clock_ghz_mean;
    int64_t workgroups;  /* pass-2 workgroups whose clock was resolved (>= 1 us) */
    int32_t fused;
    int32_t groups;  /* pipelined batch: pair groups (0: not pipelined) */
} gsa_full_timing;
int gsa_set_full_timing(gsa_ctx* ctx, int32_t on);
int gsa_last_full_timing(gsa_ctx* ctx, gsa_full_timing* out);

/* Measurement and test aid, not part of the reference's interface: which instance the last call on
 * this context ran, as the host decided it at the launch (after every fallback), so a test or a
 * probe that sets a knob can see that the knob reached the library.  Fills, score calls and the
 * device trace each overwrite the whole record; fields that do not apply to a kind are 0. */
enum gsa_launch_kind
{
    GSA_LAUNCH_NONE = 0,
    GSA_LAUNCH_FULL_LANE = 1,       /* one-pass lane fill (nw_lane.hip) */
    GSA_LAUNCH_FULL_FUSED = 2,      /* two-pass full fill, both passes in one launch */
    GSA_LAUNCH_FULL_TWO_LAUNCH = 3, /* two-pass full fill, pass 1 and the expansion as two launches */
    GSA_LAUNCH_SPARSE_KROW = 4,     /* K-rows sparse fill (nw_krow.hip) */
    GSA_LAUNCH_SPARSE_STRIP = 5,    /* strip sparse fill (nw_strip.hip) */
    GSA_LAUNCH_SCORE_KROW = 6,      /* K-rows score kernel */
    GSA_LAUNCH_SCORE_STRIP = 7,     /* strip kernel's score modes */
    GSA_LAUNCH_SCORE_SCAN = 8,      /* row scan (nw_scan.hip) */
    GSA_LAUNCH_TRACE_SPARSE = 9,    /* gsa_trace_sparse_dev */
    GSA_LAUNCH_SCORE_LANES = 10     /* database search, a subject per group of lanes (nw_lanes.hip):
                                     * npairs = subjects on that kernel, tickets = wave tasks, k = query
                                     * rows per lane, ns = waves per workgroup */
};
typedef struct gsa_launch_info
{
    int32_t kind;        /* enum gsa_launch_kind */
    int32_t ns, k;       /* strips per workgroup and rows per lane as passed to the launcher (lane fill:
                          * ns lane strips, k = 1; a full two-pass fill: pass 1's; strip kernel: 4, 1) */
    int32_t q8;          /* K-rows kernels: 0 = the int16 profile only, 1 = the int8 instance with the
                          * int16 one behind it */
    int32_t q8_declined; /* 1: the int8 instance declined the table and the int16 one ran */
    int32_t staged;      /* fused full fill: row 64m through the storer wave */
    int32_t mlsppt;      /* sparse fill launched by gsa_align_sparse_pt */
    int32_t both_ends;   /* score: the pair ran from both ends */
    int32_t npairs;
    int32_t pair_major;  /* a batch's tickets pair by pair (GSA_BATCH_ORDER=pair), not round-robin */
    int32_t trace_band;  /* device trace: the band used (GSA_TRACE_BAND), columns */
    int64_t tickets;     /* fills and strip / K-rows scores: tickets of the (pass-1) launch */
    int64_t band_tiles;  /* device trace: tiles precomputed around the diagonal (0: the walk alone) */
} gsa_launch_info;
/* errorInvalidValue: nothing launched yet.  q8_declined is a word the launch writes on the device, so
 * for a launch with q8 = 1 this synchronizes the stream of that launch (as gsa_debug_stamps does)
 * before it reads it. */
int gsa_last_launch(gsa_ctx* ctx, gsa_launch_info* out);

/* ---- consumers (host), the reference's L4 ----------------------------------------- */
/* NwHash1_Plain (src/nwtrace1_plain.cpp:133-154). */
uint32_t gsa_hash_full(const int32_t* score, int32_t adjrows, int32_t adjcols);
/* NwTrace1_Plain (src/nwtrace1_plain.cpp:6-131); edit string NUL-terminated if room.
 * Returns GSA_ERROR_MEMORY_ALLOCATION if `cap` is too small. */
int gsa_trace_full(const int32_t* score, const int32_t* seqY, int32_t adjrows, const int32_t* seqX,
                   int32_t adjcols, char* edit, int64_t cap, int64_t* edit_len, uint32_t* trace_hash);
/* NwTrace2_Sparse (src/nwtrace2_sparse.cpp:102-257) + the align_cost recompute of the mlsp
 * align functions (nwalign_gpu9_mlsp_diagdiagdiag.cu:713-716). */
int gsa_trace_sparse(const int32_t* tileHrowMat, const int32_t* tileHcolMat, const gsa_sparse_geom* geom,
                     const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                     const int32_t* subst, int32_t substsz, int32_t gapo, char* edit, int64_t cap,
                     int64_t* edit_len, uint32_t* trace_hash, int32_t* align_cost);
/* NwHash2_Sparse (src/nwtrace2_sparse.cpp:263-340). */
uint32_t gsa_hash_sparse(const int32_t* tileHrowMat, const int32_t* tileHcolMat, const gsa_sparse_geom* geom,
                         const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                         const int32_t* subst, int32_t substsz, int32_t gapo);
/* align_cost of a sparse result: NwTrace2_GetTileAndElemIJ + NwTrace2_AlignTile of the last
 * tile (nwalign_gpu9_mlsp_diagdiagdiag.cu:713-716). */
int32_t gsa_sparse_align_cost(const int32_t* tileHrowMat, const int32_t* tileHcolMat, const gsa_sparse_geom* geom,
                              const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                              const int32_t* subst, int32_t substsz, int32_t gapo);

/* ---- device-side verification ------------------------------------- */
/* The reference compares a GPU fill only through align_cost and the score / trace hashes, so
 * sparse header values off the trace path are never checked (nwtrace2_sparse.cpp:263-340).
 * These check EVERY output value against the recurrence (nwalign_cpu1_st_row.cpp:4-10) on the
 * device: a sparse result by tile consistency (each tile recomputed from its own header row
 * and column must reproduce the headers of the tiles below and to the right; row 0 / column 0
 * must be j*g / i*g; the two copies of each tile corner must agree), a full matrix cell by
 * cell against its stored neighbours.  Zero mismatches implies every value is exact.
 * Synchronous on `stream`; inputs are device pointers. */
typedef struct gsa_check_result
{
    int64_t checked;    /* values compared */
    int64_t mismatches; /* values inconsistent with the recurrence or the boundary */
    int64_t first;      /* smallest mismatching index, -1 if none: full = i*adjcols+j;
                           sparse = index into tileHrowMat, or hrowElems + index into tileHcolMat */
} gsa_check_result;
int gsa_check_sparse_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                         const int32_t* subst, int32_t substsz, int32_t gapo, const gsa_sparse_geom* geom,
                         const int32_t* tileHrowMat, const int32_t* tileHcolMat, gsa_check_result* out,
                         void* stream);
int gsa_check_full_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, const int32_t* score,
                       gsa_check_result* out, void* stream);
/* As gsa_check_full_dev for a matrix with row pitch ld (>= adjcols, gsa_fill_full_pitched_dev);
 * `first` is still i*adjcols+j. */
int gsa_check_full_pitched_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX,
                               int32_t adjcols, const int32_t* subst, int32_t substsz, int32_t gapo,
                               const int32_t* score, int32_t ld, gsa_check_result* out, void* stream);

/* The plain family's consumers over a matrix that stays in HBM (row pitch ld >= adjcols; ld =
 * adjcols for gsa_fill_full_dev output), so a 100k x 100k matrix (40 GB) is hashed and traced
 * without a host copy of it.  Results are identical to gsa_hash_full / gsa_trace_full of the
 * same matrix.  Both wait for `stream` first and are synchronous.
 * gsa_hash_full_dev: NwHash1_Plain (src/nwtrace1_plain.cpp:133-154); the hash is one serial chain
 *   over every cell, folded on the host while rows stream through two pinned buffers.
 * gsa_trace_full_dev: NwTrace1_Plain (src/nwtrace1_plain.cpp:6-131) -- the walk reads blocks of
 *   the matrix around its position; seqY/seqX are device pointers; align_cost = the last cell. */
int gsa_hash_full_dev(gsa_ctx* ctx, const int32_t* score, int32_t adjrows, int32_t adjcols, int32_t ld,
                      uint32_t* hash, void* stream);
int gsa_trace_full_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* score, int32_t ld, char* edit, int64_t cap, int64_t* edit_len,
                       uint32_t* trace_hash, int32_t* align_cost, void* stream);

/* NwTrace2_Sparse (src/nwtrace2_sparse.cpp:102-257) on the device: the walk and its tile
 * recomputes run on the GPU from device-resident headers; outputs (edit string, trace hash,
 * align_cost) are identical to gsa_trace_sparse.  Synchronous on `stream`. */
int gsa_trace_sparse_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                         const int32_t* subst, int32_t substsz, int32_t gapo, const gsa_sparse_geom* geom,
                         const int32_t* tileHrowMat, const int32_t* tileHcolMat, char* edit, int64_t cap,
                         int64_t* edit_len, uint32_t* trace_hash, int32_t* align_cost, void* stream);

/* ---- score-only NW / SW, linear or affine gaps (BASELINE configs[4]) ---- */
/* Not in the reference (README.md:7-23 marks AG/SW unimplemented; --gapeCost is unused,
 * cmd_parser.cpp:143).  Semantics: oracle/score_oracle.c --
 *   E = max(E_left + gape, H_left + gapo), F = max(F_up + gape, H_up + gapo),
 *   H = max(H_diag + s, E, F [, 0 if local]); a gap of length L costs gapo + (L-1)*gape;
 *   global: score = H[R][C], boundaries gapo + (k-1)*gape; local: max over H, end = first
 *   cell in row-major order.  gapo == gape == g is the reference's NW-LG.  Requires
 *   gapo <= gape <= 0.  Synchronous.
 * Accepted value range, the same for all six device entry points below and for gsa_score: with
 * smax the largest |table value| (at least 1), R and C the letter counts and
 *   B = smax min(R, C) + |gapo| + (R + C) |gape|      (no |H| exceeds it)
 * a global pair needs B + |gapo| < 2^29 and a local pair B < 2^30; a local pair also needs
 * ceil(log2((R + 1)(C + 1))) + bits(min(smax min(R, C), 2^31 - 1)) <= 63 for its end-cell key.
 * A pair outside is errorInvalidValue before anything is enqueued; every pair inside is computed
 * exactly, on whichever kernel takes it ("Value-range guards").  The kernels keep
 * -2^29 for minus infinity: the global bound is what keeps every true H + gapo above it; local
 * values never fall below 0, so nothing that comes from it can win there. */
/* gsa_score_dev reads the substitution table back in stream order (it sizes the value range
 * from it) before its launch; the score kernels report errors in a control word of their own, so
 * the fills' sticky error word is left for the caller's gsa_sync.  Global scores of long pairs run
 * from both ends (the top rows forward, the bottom rows reversed, in one launch; the pair
 * transposed when only adjcols-1 suits the split); local ones too, by rows only, with a third
 * pair (the bottom rows forward from a fresh border) for the end cell and a second launch when
 * an alignment through the split row decides the result: same results, context scratch grows by
 * ~4 (adjcols + adjrows) ints and, local, by the granules of one more pass. */
typedef struct gsa_score_result
{
    int32_t score;
    int64_t i_end, j_end;  /* local: where the maximum first occurs; global: (adjrows-1, adjcols-1) */
    float calc_kernel_ms;  /* hipEvent time of the fill: for scores split in two halves (from both
                            * ends) the prep, fill and combine kernels, and a local
                            * pair's second launch when it needed one */
} gsa_score_result;
/* Accepted range: global B + |gapo| < 2^29, local B < 2^30 (above); else errorInvalidValue. */
int gsa_score_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                  const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                  gsa_score_result* out, void* stream);
/* Many pairs in ONE persistent launch: `pairs` is a host array of `npairs` entries of which only
 * seqY, adjrows, seqX and adjcols are read (device pointers, as gsa_score_dev's; two entries may
 * name the same sequences), `out` a host array of `npairs` results.  out[p] is what gsa_score_dev
 * returns for pair p alone -- score, and end cell with the same first-in-row-major tie rule --
 * except that out[p].calc_kernel_ms is 0; *batch_kernel_ms (may be null) gets the hipEvent time of
 * the whole call's kernels.  Synchronous, like gsa_score_dev: the results are in `out` on return.
 * Every pair gets tickets of 64 K x 4 rows of the K-rows score kernel (K = 4 rows per lane in every
 * mode, the measured winner for throughput; GSA_SCORE_K = 2 / 4 forces it), the tickets of all pairs run round-robin, longest pair first, as the
 * batched fills' do (GSA_BATCH_ORDER=pair: pair by pair), and a small kernel behind the fill
 * decodes every pair's result words, which the host reads with one copy.  No pair is split in two
 * halves here: the other pairs keep the chip busy.  A pair with an empty sequence is answered on the
 * host.  Fallback rule -- the results never depend on the path a pair took: a pair outside the
 * kernel's value range (gsa_score_dev's own test, per pair), or one the kernel reports as too large
 * (a local score >= 2^26), runs through gsa_score_dev's single-pair path after the batch launch;
 * the whole batch takes that path, pair by pair, when the kernel reports a table outside int16,
 * when its profile does not fit LDS, or with GSA_SCORE_SCAN=1 or GSA_SCORE_KERNEL=strip.
 * gapo > gape, gape > 0, npairs < 1, a null pointer or an entry with adjrows or adjcols < 1 is
 * errorInvalidValue before anything is enqueued.  The kernel's errors go to the score kernels' own
 * control word, as gsa_score_dev's.  gsa_last_launch then reports the batch launch (kind
 * GSA_LAUNCH_SCORE_KROW, npairs as passed, the tickets of all pairs, k, q8, pair_major), or the
 * last single-pair launch when a pair took the fallback.
 * Pairs much shorter than a ticket leave most of its lanes idle.
 * Accepted range: gsa_score_dev's, for every pair (global B + |gapo| < 2^29, local B < 2^30); one
 * pair outside it makes the call errorInvalidValue before anything is enqueued. */
int gsa_score_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                        int32_t substsz, int32_t gapo, int32_t gape, int32_t local, gsa_score_result* out,
                        float* batch_kernel_ms, void* stream);
/* One query against a database of subjects, score-only; semantics of gsa_score_dev with
 * seqY = query, seqX = subject s.  db is ONE device buffer holding the subjects back to back, each
 * with its own header element 0 in front; subject s is db + db_off[s], adjcols = db_off[s+1] - db_off[s].
 * db_off is a HOST array of nsubj + 1 strictly increasing offsets (every subject has at least its
 * header).  out is a host array of nsubj results: out[s] is exactly what gsa_score_dev returns for
 * (query, subject s) -- score, and for local the first maximal cell in row-major order -- with
 * calc_kernel_ms = 0; *kernel_ms (may be null) gets the hipEvent time of the call's kernels.
 * Synchronous.
 * Subjects of at most Lmax letters (GSA_DB_MAXC=n overrides it, at most 8191) run on
 * the lane kernel (nw_lanes.hip): every subject on 16 lanes of a wave, no wave waiting for another.
 * The results never depend on the path: longer subjects, local pairs whose score bound
 * (largest |table value| x the shorter length) reaches 2^18, and every subject when the query's
 * profile does not fit LDS or with GSA_DB_LANES=0 run through gsa_score_batch_dev's path, as a pair
 * list built inside the call, before the lane launch.  A subject with no letters, or an empty query,
 * is answered on the host.  A null pointer, nsubj < 1, adjq < 1, an offset that does not increase,
 * gapo > gape, gape > 0, substsz outside 1..32 or a pair outside every kernel's value range is
 * errorInvalidValue before anything is enqueued.  The fills' sticky error word is left alone.
 * gsa_last_launch reports the lane launch (kind GSA_LAUNCH_SCORE_LANES) when any subject took it,
 * else what the other path reports.
 * Accepted range: gsa_score_dev's, for the query against every subject with letters (global
 * B + |gapo| < 2^29, local B < 2^30). */
int gsa_score_db_dev(gsa_ctx* ctx, const int32_t* query, int32_t adjq, const int32_t* db,
                     const int64_t* db_off, int32_t nsubj, const int32_t* subst, int32_t substsz,
                     int32_t gapo, int32_t gape, int32_t local, gsa_score_result* out,
                     float* kernel_ms, void* stream);

/* Alignments of chosen subjects of a database search. */
typedef struct gsa_align_db_result {
    int32_t score;
    int32_t status;              /* 0 aligned; 1 outside the trace kernel's limits: score and end cell only,
                                    empty CIGAR; 2 CIGAR did not fit cigar_cap */
    int64_t i_start, j_start, i_end, j_end;
    int64_t cigar_off, cigar_len; /* into `cigar`; NUL-terminated there, the NUL not counted */
} gsa_align_db_result;

typedef struct gsa_align_db_info {  /* what the call ran; optional out-parameter */
    int32_t lane_hits;      /* hits traced on the device */
    int32_t unsupported;    /* hits with status 1 */
    int32_t chunks;         /* fill + walk launch pairs */
    int64_t tasks;          /* wave tasks over all chunks */
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    float fill_ms, walk_ms; /* hipEvent time of the fill and of the walk launches, summed over the chunks */
} gsa_align_db_info;

/* The alignments of nhits subjects of a database, traced on the device.  query, db, db_off, nsubj,
 * subst, substsz, gapo, gape, local: exactly as gsa_score_db_dev takes them.  hits is a HOST array of
 * nhits subject indices (0 ... nsubj - 1), in any order; a subject may be named twice.  out is a host
 * array of nhits results, out[h] for hits[h].  Synchronous.
 * Semantics: the recurrences and boundaries of gsa_score_dev; score, i_end and j_end are exactly what
 * gsa_score_db_dev returns for that subject (local: the first maximal cell in row-major order).  The
 * path is walked backwards from the end cell, starting in state H.  State H at cell i, j: local and
 * H = 0: stop; else H = H[i-1][j-1] + s: diagonal; else H = F[i][j]: state F; else state E (row 0 of a
 * global alignment is E only, column 0 F only).  State F: a vertical move to i-1, j; the gap was
 * extended (stay in F) iff F[i-1][j] + gape > H[i-1][j] + gapo, strictly, else opened (back to H).
 * State E: the same along the row.  Global alignments stop at cell 0, 0.  i_start, j_start is the cell
 * the path starts at: the aligned letters are query i_start+1 ... i_end and subject j_start+1 ... j_end.
 * A local alignment of score 0 starts and ends at 0, 0 with an empty CIGAR.
 * CIGAR: forward order, run-length encoded with decimal counts: '=' diagonal on equal letters, 'X'
 * diagonal on different letters, 'I' vertical (a query letter only), 'D' horizontal (a subject letter
 * only).  The strings go into `cigar` (cigar_cap bytes), NUL-terminated, back to back in hit order;
 * a hit's offset does not depend on cigar_cap.  A string that does not fit is left out (status 2,
 * the cells are still valid); *cigar_need (may be null) gets the bytes all strings need, so that a
 * caller with a short buffer can call again; 2 (R + C) + 1 bytes per hit always suffice.
 * Every traced hit keeps 4 bits per cell of move codes on the device until its path is walked:
 * ceil(R / 384) x 384 x (C + 1) / 2 bytes.  scratch_limit is the bytes of codes the call may hold at
 * once; 0 is the default, 256 MiB.  The hits are taken longest first and cut into chunks that fit;
 * each chunk is one fill and one walk launch (nw_lanes_trace.hip) and one copy back.  The scratch is
 * counted in the peaks of gsa_mem_stats.
 * Status 1 -- score and end cell from gsa_score_batch_dev's path, no CIGAR: a hit whose codes alone
 * exceed the limit, a subject of more than 8191 letters, a query whose profile does not fit LDS, a
 * local pair whose score bound reaches 2^18, a pair whose value bound (largest |table value| x the
 * shorter length + |gapo| + (R + C) |gape|) reaches 2^26.  No score depends on the route.  A subject with no
 * letters is answered on the host (global: R x 'I'; local: score 0, empty CIGAR), as is an empty query.
 * Everything gsa_score_db_dev rejects, a null hits with nhits > 0, a hit outside 0 ... nsubj - 1, a
 * negative nhits, scratch_limit or cigar_cap, a null out, a null cigar with cigar_cap > 0 or a null
 * context is errorInvalidValue before anything is enqueued; nhits = 0 succeeds with nothing launched.
 * *info (may be null) says what the call ran.  This call adds no launch kind and no knob: the record
 * of gsa_last_launch is left untouched, also by the status 1 hits' score launches.  *kernel_ms (may be
 * null) gets the hipEvent time of all kernels of the call.
 * Accepted range: gsa_score_db_dev's, over the whole database and not the hits alone (global
 * B + |gapo| < 2^29, local B < 2^30).  The trace fills keep -2^27 for minus infinity, which the
 * status 1 bound B < 2^26 keeps below every true H + gapo. */
int gsa_align_db_dev(gsa_ctx* ctx, const int32_t* query, int32_t adjq, const int32_t* db, const int64_t* db_off,
                     int32_t nsubj, const int32_t* hits, int32_t nhits, const int32_t* subst, int32_t substsz,
                     int32_t gapo, int32_t gape, int32_t local, int64_t scratch_limit, gsa_align_db_result* out,
                     char* cigar, int64_t cigar_cap, int64_t* cigar_need, gsa_align_db_info* info,
                     float* kernel_ms, void* stream);

/* The alignment of one long pair. */
typedef struct gsa_align_pair_info {  /* what the call ran; optional out-parameter */
    int32_t strip_rows;     /* TR: rows of a strip, the score kernel's ticket (512 or 1024); 0: that kernel did not run */
    int32_t strips;         /* strips that hold the rows 1 ... i_end */
    int32_t strips_filled;  /* strips filled with move codes, over all chunks */
    int32_t chunks;         /* fill + walk launch pairs */
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    float score_ms, fill_ms, walk_ms; /* hipEvent time of the score launch, and of the fill and the walk launches
                                         summed over the chunks */
    int32_t pad0;
} gsa_align_pair_info;

/* The alignment of one pair of any length the K-rows score kernel takes, traced on the device.  seqY
 * (the query, down the rows), adjrows, seqX (the subject, along the columns), adjcols, subst, substsz,
 * gapo, gape, local: exactly as gsa_score_dev takes them.  out is one host result.  Synchronous.
 * Semantics: gsa_align_db_dev's, word for word -- the recurrences, boundaries and end cell of
 * gsa_score_dev (score, i_end and j_end are what gsa_score_dev returns for the same arguments; local:
 * the first maximal cell in row-major order), the walk from the end cell in state H with diagonal
 * before F before E and a gap extended only when that is strictly better than opening, i_start /
 * j_start, the CIGAR letters '=', 'X', 'I', 'D', and the CIGAR buffer rules: one NUL-terminated string
 * at cigar[0], status 2 when it does not fit cigar_cap (the cells are still valid), *cigar_need (may be
 * null) the bytes it needs, 2 (R + C) + 1 always enough.  A pair with an empty side is answered on
 * the host as gsa_align_db_dev answers it.
 * How: the K-rows score kernel runs the pair in one direction (no split from both ends) and leaves
 * the bottom row of each of its tickets of TR rows (512, NW with linear gaps 1024) in its hand-off
 * rows.  With those exact, every strip of TR rows is independent: the strips from i_end's upwards are
 * refilled with 4-bit move codes, one wave per strip, all at once (nw_pair_trace.hip), and one lane
 * walks the codes.  A strip's codes over the columns 1 ... j_end take j_end x TR / 2 bytes.
 * scratch_limit is the bytes of codes the call may hold at once; 0 is the default, 2 GiB (a
 * 64k x 64k pair).  When the strips do not all fit they are taken bottom-up in chunks of consecutive
 * strips, a fill and a walk launch and one small copy back per chunk; a later chunk is filled only
 * up to the column where the walk left the one below, and a local walk that ends inside a chunk
 * ends the call.  The scratch is counted in the peaks of gsa_mem_stats.
 * Status 1 -- score and end cell from gsa_score_dev's path, no CIGAR: a pair the K-rows score kernel
 * does not run (a table outside int16 after the shift, a local score of 2^26 or more, a local pair
 * the strip kernels do not take, LDS, GSA_SCORE_KERNEL=strip, GSA_SCORE_SCAN=1), a pair whose value
 * bound (largest |table value| x the shorter length + |gapo| + (R + C) |gape|) reaches 2^26, a pair
 * whose single strip exceeds scratch_limit.  No score depends on the route.
 * Everything gsa_score_dev rejects (its value range included), a negative scratch_limit or cigar_cap,
 * a null out, a null cigar with cigar_cap > 0 or a null context is errorInvalidValue before anything
 * is enqueued.  *info (may be null) says what the call ran.  This call adds no launch kind and no
 * knob: the record of gsa_last_launch is left untouched.  *kernel_ms (may be null) gets the hipEvent
 * time of all kernels of the call. */
int gsa_align_pair_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                       int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                       int64_t* cigar_need, gsa_align_pair_info* info, float* kernel_ms, void* stream);

/* The alignments of a batch of long pairs in one call. */
typedef struct gsa_align_batch_info {  /* what the call ran; optional out-parameter */
    int32_t batch_pairs;    /* pairs traced by the batched route */
    int32_t alone_pairs;    /* pairs passed on to gsa_align_pair_dev's path, one by one */
    int32_t host_pairs;     /* pairs answered on the host: an empty side, a local score of 0 */
    int32_t strip_rows;     /* TR: rows of a strip, the batched score kernel's ticket (1024; 512 with
                               GSA_SCORE_K=2); 0: that kernel did not run */
    int32_t strips;         /* strips that hold the rows 1 ... i_end, over all batch pairs */
    int32_t strips_filled;  /* strips filled with move codes, over all rounds */
    int32_t rounds;         /* fill + walk launch pairs */
    int32_t pad0;
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    float score_ms, fill_ms, walk_ms; /* hipEvent time of the batched score launch, and of the fill and the walk
                                         launches summed over the rounds (the pairs that went alone: kernel_ms only) */
    int32_t pad1;
} gsa_align_batch_info;

/* The alignments of npairs pairs, each of any length the K-rows score kernel takes, traced on the
 * device together.  pairs is a HOST array as gsa_score_batch_dev takes it; only seqY, adjrows, seqX and
 * adjcols are read.  subst, substsz, gapo, gape, local: as gsa_score_batch_dev takes them.  out is a
 * host array of npairs results.  Synchronous.
 * Semantics: out[p] is, field for field, what gsa_align_pair_dev returns for pair p alone -- score,
 * both cells and the CIGAR, the same recurrences and tie rule -- whatever the strip height, the round,
 * the pair's neighbours in the batch and max_workgroups.  The CIGAR buffer follows gsa_align_db_dev's
 * rules: the strings back to back in pair order, NUL-terminated, a pair's offset independent of
 * cigar_cap, status 2 for a string that does not fit, *cigar_need (may be null) the bytes all need.
 * How: gsa_score_batch_dev's launch scores every pair in one direction and leaves, per pair, the
 * bottom row of each ticket of TR rows in the pair's own hand-off rows.  TR is 1024 in every mode
 * (512 with GSA_SCORE_K=2), where gsa_align_pair_dev uses 512 in three of the four modes.  With those
 * rows exact every strip of every pair is independent, so the strips of many pairs are filled with
 * 4-bit move codes in one launch, one wave per strip, and the pairs' walks run side by side, one wave
 * per pair (nw_pair_trace_batch.hip).  scratch_limit is the bytes of codes the call may hold at once;
 * 0 is the default, 8 GiB.  When the strips do not all fit the call runs rounds: the pairs are taken
 * by remaining code bytes descending, each gets its lowest unfilled strip and as many above it as
 * still fit the round, for the columns up to where its walk stands; a pair for which nothing is left
 * waits.  A round is one fill launch, one walk launch and one small copy back.  max_workgroups caps
 * the grid of the fill and of the walk (0: all resident), as in gsa_align_db_multi_dev.  The scratch
 * is counted in the peaks of gsa_mem_stats.
 * Status 0 answered on the host: a pair with an empty side (as gsa_align_db_dev answers it), a local
 * pair whose score is 0 (cells 0, 0, empty CIGAR).
 * Status 1 -- score and end cell, no CIGAR -- under gsa_align_pair_dev's conditions, per pair: a value
 * bound (largest |table value| x the shorter length + |gapo| + (R + C) |gape|) of 2^26 or more, a pair
 * the K-rows score kernel does not take or flags, a pair whose single strip, of this call's TR rows
 * over its columns 1 ... j_end, exceeds scratch_limit.  The strip height being 1024 here and 512 there
 * in three modes, the last condition can differ between the two calls at a limit between the two
 * strip sizes, and nowhere else.  The pairs the batched score launch did not run or flagged go through
 * gsa_align_pair_dev's path one by one afterwards.  No score depends on the route.
 * Everything gsa_score_batch_dev rejects, a negative scratch_limit, cigar_cap or max_workgroups, a null
 * out, a null cigar with cigar_cap > 0 or a null context is errorInvalidValue before anything is
 * enqueued.  *info (may be null) says what the call ran.  This call adds no launch kind and no knob:
 * the record of gsa_last_launch is left untouched.  *kernel_ms (may be null) gets the hipEvent time of
 * all kernels of the call. */
int gsa_align_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                        int32_t substsz, int32_t gapo, int32_t gape, int32_t local, int32_t max_workgroups,
                        int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                        int64_t* cigar_need, gsa_align_batch_info* info, float* kernel_ms, void* stream);

/* Many queries against one database in one call. */
typedef struct gsa_db_hit { int32_t subject, score, i_end, j_end; } gsa_db_hit;

typedef struct gsa_score_db_multi_info {  /* what the call ran; optional out-parameter */
    int32_t lane_queries, other_queries;  /* queries on the multi-query lane kernel / sent whole through gsa_score_db_dev's path */
    int32_t launches;                     /* lane launches (chunks x sweep classes) */
    int32_t workgroups;                   /* grid of the last lane launch */
    int64_t lane_pairs, units, profile_builds, result_bytes; /* result_bytes: peak device bytes of results held at once */
    float lanes_ms, select_ms;            /* hipEvent time of the lane launches and of the ranking, summed over the chunks */
} gsa_score_db_multi_info;

/* nq queries against the nsubj subjects of a database, score-only.  db, db_off, nsubj, subst, substsz,
 * gapo, gape, local: exactly as gsa_score_db_dev takes them.  queries and q_off follow the conventions
 * of db and db_off: ONE device buffer holding the queries back to back, each with its header element,
 * and a HOST table of nq + 1 strictly increasing offsets.  Synchronous.
 * Semantics: the result of (query q, subject s) -- score and end cell, local: the first maximal cell
 * in row-major order -- is exactly what gsa_score_db_dev returns for query q and subject s; it never
 * depends on the path.  scores (host, int32[nq * nsubj], may be null) gets the scores, row q for query
 * q.  hits (host, gsa_db_hit[nq * ntop], ntop = min(top, nsubj); may be null when top = 0) gets, per
 * query, its ntop best subjects by (score descending, subject index ascending), ranked on the device.
 * At least one of the two is non-null.
 * All (query, subject) pairs of the subjects the lane kernel takes (1 ... Lmax letters, GSA_DB_MAXC as
 * in gsa_score_db_dev) run in the task space of one persistent launch per sweep class (queries of
 * 1 ... 384, 385 ... 768, ... letters) of nw_lanes_multi.hip: units of gsa_score_db_multi_unit() wave
 * tasks of one query, query-major, longest query first, claimed by workgroups that rebuild the query
 * profile in LDS when a unit's query is not the resident one.  max_workgroups: 0 as many workgroups as
 * are resident, n > 0 at most n.  Pairs with an empty side are answered on the host; subjects past
 * Lmax go through gsa_score_batch_dev's path, per query; a query whose profile does not fit LDS, one
 * with a lane subject past the local key's bound (largest |table value| x the shorter length >= 2^18),
 * and every query with GSA_DB_LANES=0 goes whole through gsa_score_db_dev's path.  Those results are
 * written into the device matrix by a scatter kernel before the ranking.
 * The results (16 bytes per pair) are held on the device for a chunk of consecutive queries at a
 * time: scratch_limit is the bytes of result matrix held at once, 0 the default of 256 MiB; a limit
 * below one query's row (16 nsubj bytes) is errorInvalidValue.  Each chunk is its lane launches, a
 * ranking (top > 0; its keys take another 16 bytes per pair and the sort's own storage) and one copy
 * back of the hits and / or score rows.  All device memory is the context's and counted in
 * gsa_mem_stats.
 * Everything gsa_score_db_dev rejects, for either offset table, nq < 1, a negative top, max_workgroups
 * or scratch_limit, scores and hits both null, or hits null with top > 0 and scores null, is
 * errorInvalidValue before anything is enqueued.  The call adds no launch kind and no knob: the record
 * of gsa_last_launch is left untouched and *info (may be null) says what ran; the fills' sticky error
 * word is left alone.  *kernel_ms (may be null) gets the hipEvent time of all kernels of the call.
 * Accepted range: gsa_score_dev's for the longest query against the longest subject (global
 * B + |gapo| < 2^29, local B < 2^30), which bounds every pair's. */
int gsa_score_db_multi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                           const int32_t* db, const int64_t* db_off, int32_t nsubj,
                           const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                           int32_t top, int32_t max_workgroups, int64_t scratch_limit,
                           int32_t* scores, gsa_db_hit* hits,
                           gsa_score_db_multi_info* info, float* kernel_ms, void* stream);
/* Wave tasks (of four subjects) in a unit of gsa_score_db_multi_dev: a compile-time constant. */
int32_t gsa_score_db_multi_unit(void);

/* The alignments of many queries' hits in one call. */
typedef struct gsa_align_db_multi_info {  /* what the call ran; optional out-parameter */
    int32_t lane_hits;      /* hits traced on the device */
    int32_t unsupported;    /* hits with status 1 */
    int32_t chunks;         /* chunks: one walk launch and one copy back each */
    int32_t launches;       /* fill launches (chunks x sweep classes) */
    int32_t workgroups;     /* grid of the last fill launch */
    int32_t lane_queries;   /* queries with traced hits, summed over the chunks */
    int64_t tasks, units;   /* wave tasks and units over all chunks */
    int64_t profile_builds; /* query profiles built in LDS, over all launches */
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    float fill_ms, walk_ms; /* hipEvent time of the fill and of the walk launches, summed over the chunks */
} gsa_align_db_multi_info;

/* The alignments of nhits (query, subject) pairs, traced on the device.  queries, q_off, nq, db, db_off,
 * nsubj, subst, substsz, gapo, gape, local: exactly as gsa_score_db_multi_dev takes them.  hit_query and
 * hit_subject are HOST arrays of nhits indices (0 ... nq - 1 and 0 ... nsubj - 1), in any order; a pair
 * may be named twice.  out is a host array of nhits results.  Synchronous.
 * Semantics: out[h] is, field for field, what gsa_align_db_dev returns for query hit_query[h] and the
 * single hit hit_subject[h] under the same scratch_limit: score, status, both cells and the CIGAR.
 * The status 1 conditions of gsa_align_db_dev are evaluated per pair with that hit's query, and the
 * status 1 hits of all queries take one gsa_score_batch_dev pass; pairs with an empty side are answered
 * on the host.  The CIGAR buffer follows gsa_align_db_dev's rules: strings back to back in hit order,
 * NUL-terminated, offsets independent of cigar_cap, status 2 for a string that does not fit,
 * *cigar_need the bytes all of them need.
 * The traced hits are ordered by query length (longest first), query, and subject length (longest
 * first), and cut greedily into chunks whose move codes fit scratch_limit (0: 256 MiB).  In a chunk the
 * hits of one query form wave tasks of up to four hits and units of up to gsa_align_db_multi_unit()
 * consecutive tasks; the units of one sweep class (queries of 1 ... 384, 385 ... 768, ... letters) are
 * one persistent fill launch of nw_lanes_trace_multi.hip, whose workgroups claim units and rebuild the
 * query profile in LDS when a unit's query is not the resident one; one walk launch and one copy back
 * serve the whole chunk.  max_workgroups: 0 as many workgroups as are resident, n > 0 at most n.  The
 * scratch is gsa_align_db_dev's and counted in gsa_mem_stats.
 * Everything gsa_align_db_dev rejects, for either offset table, nq < 1, a hit index out of range, a null
 * hit_query or hit_subject with nhits > 0, a negative nhits, max_workgroups, scratch_limit or cigar_cap,
 * or the longest query against the longest subject outside every kernel's value range is
 * errorInvalidValue before anything is enqueued; nhits = 0 succeeds with nothing launched.  The call
 * adds no launch kind and no knob: the record of gsa_last_launch is left untouched and *info (may be
 * null) says what ran.  *kernel_ms (may be null) gets the hipEvent time of all kernels of the call.
 * Accepted range: gsa_score_db_multi_dev's (the longest query against the longest subject: global
 * B + |gapo| < 2^29, local B < 2^30). */
int gsa_align_db_multi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                           const int32_t* db, const int64_t* db_off, int32_t nsubj,
                           const int32_t* hit_query, const int32_t* hit_subject, int32_t nhits,
                           const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
                           int32_t max_workgroups, int64_t scratch_limit, gsa_align_db_result* out,
                           char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                           gsa_align_db_multi_info* info, float* kernel_ms, void* stream);
/* Wave tasks (of up to four hits) in a unit of gsa_align_db_multi_dev: a compile-time constant. */
int32_t gsa_align_db_multi_unit(void);

/* Database search, semi-global mode: the whole query within each subject.
 * The alignment shape is neither of gsa_score_db_multi_dev's two: every query letter is aligned, and
 * the subject's unaligned head and tail cost nothing (an adapter, primer or barcode in every read, a
 * domain in every protein).  With R query and C subject letters and the Gotoh recurrences of
 * "score-only NW / SW" above, without the zero floor:
 *   row 0 is free:        H(0, j) = 0, E(0, j) = F(0, j) = minus infinity, j = 0 ... C;
 *   column 0 is global:   H(i, 0) = F(i, 0) = gapo + (i - 1) gape, E(i, 0) = minus infinity, i >= 1;
 *   score = max over j = 0 ... C of H(R, j) -- column 0, the all-insert alignment, is a candidate;
 *   end cell: i_end = R, j_end the SMALLEST j that attains the score.
 * Scores may be negative.  A subject without letters against a query with some: score
 * gapo + (R - 1) gape, end cell (R, 0); a query without letters: score 0, end cell (0, 0); both are
 * answered on the host.
 *
 * gsa_score_db_multi_semi_dev takes gsa_score_db_multi_dev's arguments without local; queries, q_off,
 * nq, db, db_off, nsubj, subst, substsz, gapo, gape, top, max_workgroups, scratch_limit, scores, hits,
 * info, kernel_ms and stream mean what they mean there: the same chunks of result rows, the same
 * ranking by (score descending, subject index ascending) on the device, the same device buffers
 * (counted in gsa_mem_stats).  *info is a gsa_score_db_multi_info with other_queries = 0.  The pairs run
 * on nw_lanes_semi.hip, one persistent launch per sweep class with gsa_score_db_multi_unit() tasks per
 * unit.
 * This mode has no second path: a pair runs on the lane kernels or the call is refused.  It is
 * errorInvalidValue, before anything is enqueued, when any (query, subject) pair with letters on both
 * sides has a subject of more than 8191 letters, a query whose profile (4 substsz (384 ceil(R / 384) + 4)
 * bytes) does not fit the LDS a workgroup may have, or a value bound
 * B = smax min(R, C) + |gapo| + (R + C) |gape| >= 2^18 (smax: the largest |table value|); as all
 * three grow with R and C, the longest query against the longest subject decides.  GSA_DB_MAXC and
 * GSA_DB_LANES do not apply.  Everything gsa_score_db_multi_dev rejects is rejected here too.  The call
 * adds no launch kind and no knob: the record of gsa_last_launch is left untouched and the fills'
 * sticky error word is left alone. */
int gsa_score_db_multi_semi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                const int32_t* db, const int64_t* db_off, int32_t nsubj,
                                const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                                int32_t top, int32_t max_workgroups, int64_t scratch_limit,
                                int32_t* scores, gsa_db_hit* hits,
                                gsa_score_db_multi_info* info, float* kernel_ms, void* stream);

/* The semi-global alignments of nhits (query, subject) pairs, traced on the device: the arguments of
 * gsa_align_db_multi_dev without local, the same result struct, CIGAR buffer rules (strings back to
 * back in hit order, status 2 for one that does not fit, *cigar_need), chunks by scratch_limit
 * (0: 256 MiB), *info and *kernel_ms.
 * Semantics: score and end cell (R, j_end) are gsa_score_db_multi_semi_dev's for the pair.  The walk
 * goes backwards from (R, j_end) in state H under gsa_align_db_dev's rules -- diagonal before F before
 * E at equal value, a gap extended only when that is strictly better than opening, column 0 F only --
 * and stops as soon as it is in row 0: i_start = 0, j_start the column it stopped in; no 'D' is
 * emitted in row 0, so the subject's head and tail stay out of the CIGAR.  A subject without letters
 * gives R x 'I' from (0, 0) to (R, 0); a query without letters score 0, all cells (0, 0) and an empty
 * CIGAR; both on the host.
 * No hit is status 1 (info->unsupported = 0): the call is errorInvalidValue, before anything is
 * enqueued, when a hit with letters on both sides fails one of gsa_score_db_multi_semi_dev's three
 * tests (evaluated over the hits only), or when scratch_limit is below the largest hit's move codes
 * (192 ceil(R / 384) (C + 1) bytes).  Everything gsa_align_db_multi_dev rejects is rejected here too.
 * The fill and the walk are nw_lanes_semi_trace.hip's on gsa_align_db_multi_dev's plan and buffers.  The
 * call adds no launch kind and no knob and leaves the record of gsa_last_launch untouched. */
int gsa_align_db_multi_semi_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                const int32_t* db, const int64_t* db_off, int32_t nsubj,
                                const int32_t* hit_query, const int32_t* hit_subject, int32_t nhits,
                                const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                                int32_t max_workgroups, int64_t scratch_limit, gsa_align_db_result* out,
                                char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                                gsa_align_db_multi_info* info, float* kernel_ms, void* stream);

/* Database search, overlap (dovetail) mode: a suffix of either sequence on a prefix of the other, or
 * either within the other.
 * The alignment shape of "Long pairs, overlap (dovetail) mode" below (gsa_score_overlap_dev), word for
 * word, per (query, subject) pair: an adapter that runs off a read's 3' end, a primer hanging over an
 * amplicon's end, the overlaps of a few thousand short reads, all against all.  The query has R letters
 * down the rows, the subject C letters along the columns, gapo <= gape <= 0, and
 *   row 0 and column 0 are free: H = 0, E = F = minus infinity;
 *   inside, the Gotoh recurrences of "score-only NW / SW" above, without the zero floor;
 *   candidates: the cells of row R (j = 0 ... C) and of column C (i = 0 ... R);
 *   score = the largest H among the candidates, so never negative: H(R, 0) = 0 is one;
 *   end cell: (R, the SMALLEST j that attains the score) if row R attains it, otherwise
 *   (the SMALLEST such i, C); a score of 0 therefore ends at (R, 0), and the corner (R, C) counts as
 *   row R.
 * A pair with an empty side has score 0 and end cell (R, 0), answered on the host.
 *
 * gsa_score_db_multi_overlap_dev takes gsa_score_db_multi_semi_dev's arguments, and they mean what they
 * mean there: result rows {score, i_end, j_end} per (query, subject), the same chunks of result rows
 * by scratch_limit, the same ranking by (score descending, subject index ascending) on the device,
 * top, scores, hits, *info (a gsa_score_db_multi_info with other_queries = 0), *kernel_ms and the same
 * device buffers, counted in gsa_mem_stats; no new buffer slot.  The pairs run on
 * nw_lanes_overlap.hip, one persistent launch per sweep class with gsa_score_db_multi_unit() tasks
 * per unit.
 * This mode has no second path: a pair runs on the lane kernels or the call is refused.  It is
 * errorInvalidValue, before anything is enqueued, when any (query, subject) pair with letters on both
 * sides has a subject of more than 8191 letters; a query of more than 8191 letters (the end cell's row
 * index travels in a key beside the value, as the column index does; with a small table the LDS test
 * alone would let longer queries through); a query whose profile (4 substsz (384 ceil(R / 384) + 4)
 * bytes) does not fit the LDS a workgroup may have; or a value bound
 * B = smax min(R, C) + |gapo| + (R + C) |gape| >= 2^18 (smax: the largest |table value|).  As all four
 * grow with R and C, the longest query against the longest subject decides.  GSA_DB_MAXC and
 * GSA_DB_LANES do not apply.  Everything gsa_score_db_multi_semi_dev rejects is rejected here too.  The
 * call adds no launch kind and no knob: the record of gsa_last_launch is left untouched and the fills'
 * sticky error word is left alone. */
int gsa_score_db_multi_overlap_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                   const int32_t* db, const int64_t* db_off, int32_t nsubj,
                                   const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                                   int32_t top, int32_t max_workgroups, int64_t scratch_limit,
                                   int32_t* scores, gsa_db_hit* hits,
                                   gsa_score_db_multi_info* info, float* kernel_ms, void* stream);

/* The overlap alignments of nhits (query, subject) pairs, traced on the device: the arguments of
 * gsa_align_db_multi_semi_dev, the same result struct, CIGAR buffer rules (strings back to back in hit
 * order, status 2 for one that does not fit, *cigar_need), chunks by scratch_limit (0: 256 MiB), *info
 * and *kernel_ms.
 * Semantics: score and end cell are gsa_score_db_multi_overlap_dev's for the pair.  The walk goes
 * backwards from the end cell in state H under gsa_align_db_dev's rules -- diagonal before F before E
 * at equal value, a gap extended only when that is strictly better than opening -- and stops as soon
 * as i = 0 or j = 0: (i_start, j_start) is the cell it stopped in, and nothing is emitted along a
 * border, so all four overhangs stay out of the CIGAR.  A score of 0 has start = end = (R, 0) and an
 * empty CIGAR; so has a pair with an empty side, on the host.
 * No hit is status 1 (info->unsupported = 0): the call is errorInvalidValue, before anything is
 * enqueued, when a hit with letters on both sides fails one of gsa_score_db_multi_overlap_dev's four
 * tests (evaluated over the hits only), or when scratch_limit is below the largest hit's move codes
 * (192 ceil(R / 384) (C + 1) bytes).  Everything gsa_align_db_multi_semi_dev rejects is rejected here
 * too.  The fill and the walk are nw_lanes_overlap_trace.hip's on gsa_align_db_multi_dev's plan and
 * buffers.  The call adds no launch kind and no knob and leaves the record of gsa_last_launch
 * untouched. */
int gsa_align_db_multi_overlap_dev(gsa_ctx* ctx, const int32_t* queries, const int64_t* q_off, int32_t nq,
                                   const int32_t* db, const int64_t* db_off, int32_t nsubj,
                                   const int32_t* hit_query, const int32_t* hit_subject, int32_t nhits,
                                   const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                                   int32_t max_workgroups, int64_t scratch_limit, gsa_align_db_result* out,
                                   char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                                   gsa_align_db_multi_info* info, float* kernel_ms, void* stream);
/* Long pairs, semi-global mode: a whole query within one long subject.
 * The alignment shape of "Database search, semi-global mode" above, word for word, for one pair of any
 * length the K-rows score kernel takes (a read against a contig): seqY is the query (R letters, down
 * the rows), seqX the subject (C letters, along the columns), gapo <= gape <= 0, and
 *   row 0 is free:        H(0, j) = 0, E(0, j) = F(0, j) = minus infinity, j = 0 ... C;
 *   column 0 is global:   H(i, 0) = F(i, 0) = gapo + (i - 1) gape, E(i, 0) = minus infinity, i >= 1;
 *   inside, the Gotoh recurrences without the zero floor;
 *   score = max over j = 0 ... C of H(R, j) -- column 0, the all-insert alignment, is a candidate;
 *   end cell: i_end = R, j_end the SMALLEST j that attains the score.
 * Scores may be negative.  C = 0: score gapo + (R - 1) gape, end cell (R, 0); R = 0: score 0, end cell
 * (0, 0); both are answered on the host.  A caller who wants the subject global and the query's ends
 * free swaps the two sequences and transposes the table.
 *
 * gsa_score_semi_dev takes gsa_score_dev's arguments without local and fills the same result struct.
 * Synchronous.  The pair runs in one direction on the K-rows score kernel's semi-global instances
 * (nw_kscore_semi.hip): the global step under a free row 0, with 4 rows per lane for linear gaps
 * (gapo == gape) and 2 for affine ones, as gsa_score_dev picks them for a global pair; GSA_SCORE_K and
 * GSA_KROW_Q8 are honoured as there and no other knob is read.  The strip that holds row R stores that
 * row over every column into a row buffer of 4 (C + 208) bytes in the context's scratch (counted in
 * gsa_mem_stats), a small kernel behind the fill takes its first maximum together with the analytic
 * H(R, 0), and one copy brings score and end column back.
 * This mode has no second path: the pair runs on that kernel or the call is refused.  With smax the
 * largest |table value| (at least 1) and B = smax min(R, C) + |gapo| + (R + C) |gape| it is
 * errorInvalidValue, before anything is enqueued, unless
 *   B + |gapo| < 2^29                                  (gsa_score_dev's range of a global pair),
 *   (R + C) |gape| + (gape - gapo) + smax < 2^28       (the shifted values' room in int32),
 *   the score kernel's LDS (a profile of substsz rows) fits the device, and
 *   every table value s has s - gapo - gape in (-32768, 32767]   (the kernel's int16 profile);
 * the last is checked on the host from the table, which the call reads back in stream order anyway.
 * Everything gsa_score_dev rejects is rejected here too.  The call adds no launch kind and no knob:
 * the record of gsa_last_launch is left untouched, and the kernel reports errors in the score
 * kernels' own control word, so the fills' sticky error word is left alone. */
int gsa_score_semi_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                       gsa_score_result* out, void* stream);

typedef struct gsa_align_pair_semi_info {  /* what the call ran; optional out-parameter */
    int32_t strip_rows;     /* TR: rows of a strip, the score kernel's ticket (512 or 1024) */
    int32_t strips;         /* strips that hold the rows 1 ... R */
    int32_t strips_filled;  /* strips filled with move codes, over all chunks */
    int32_t chunks;         /* fill + walk launch pairs */
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    int64_t j_window;       /* jW: codes are kept for the columns jW + 1 ... j_end only (0: from column 1) */
    float score_ms, fill_ms, walk_ms; /* hipEvent time of the score launch, and of the fill and the walk launches
                                         summed over the chunks */
    int32_t pad0;
} gsa_align_pair_semi_info;

/* The semi-global alignment of one long pair, traced on the device: gsa_align_pair_dev's arguments
 * without local, the same result struct and CIGAR buffer rules (one NUL-terminated string at cigar[0],
 * status 2 when it does not fit cigar_cap with the cells still valid, *cigar_need the bytes it needs,
 * 2 (R + C) + 1 always enough).  Synchronous.
 * Semantics: score and end cell (R, j_end) are gsa_score_semi_dev's for the pair.  The walk goes
 * backwards from (R, j_end) in state H under gsa_align_db_dev's rules -- diagonal before F before E at
 * equal value, a gap extended only when that is strictly better than opening, column 0 F only -- and
 * stops as soon as it is in row 0: i_start = 0, j_start the column it stopped in; no 'D' is emitted in
 * row 0, so the subject's head and tail stay out of the CIGAR.  C = 0: score gapo + (R - 1) gape, cells
 * (0, 0)-(R, 0), R x 'I'; R = 0: score 0, all cells (0, 0), an empty CIGAR; both on the host.
 * How: gsa_score_semi_dev's launch leaves the bottom row of each of its tickets of TR rows (512, linear
 * gaps 1024) in its hand-off rows.  Every strip of TR rows from row R's up to strip 0 -- the path
 * always reaches row 0 -- is refilled with 4-bit move codes, one wave per strip, and one lane walks the
 * codes (nw_pair_semi_trace.hip).  The codes are kept for a column window only.  With pmax = max(0,
 * largest table value) and S the score, every alignment obeys S <= pmax R + d gape for its d letters
 * of 'D', so for gape < 0 the path has at most dmax = floor((pmax R - S) / |gape|) of them and spans at
 * most R + dmax columns: with
 *   jW = max(0, j_end - R - dmax - 1)          (gape = 0: jW = 0)
 * the fill treats column jW > 0 as minus infinity below row 0 (jW = 0: the true column 0) and computes
 * the columns jW + 1 ... j_end; this is exact, ties included (nw_pair_semi_plan.h).  A strip's codes
 * take (j_end - jW) TR / 2 bytes.  scratch_limit is the bytes of codes the call may hold at once; 0 is
 * the default, 2 GiB.  When the strips do not all fit they are taken bottom-up in chunks of
 * consecutive strips, a fill and a walk launch and one small copy back per chunk; a later chunk is
 * filled only up to the column where the walk left the one below.  An end cell on column 0 (the
 * all-insert alignment) needs no codes: chunks = 0.  The scratch is counted in the peaks of
 * gsa_mem_stats.
 * No result has status 1: the mode has no second path.  The call is errorInvalidValue, before anything
 * is enqueued, for everything gsa_score_semi_dev refuses, for a pair whose value bound B reaches 2^26
 * (the fill keeps 4 x value + source), for a negative scratch_limit or cigar_cap, a null out or a null
 * cigar with cigar_cap > 0; and errorInvalidValue behind the score launch, which alone knows the
 * window, for a scratch_limit below one strip's windowed codes.  A walk that reaches column jW > 0
 * below row 0, which the bound excludes, is errorKernelFailure.  *info (may be null) says what the
 * call ran.  The call adds no launch kind and no knob and leaves the record of gsa_last_launch and the
 * fills' sticky error word alone.  *kernel_ms (may be null) gets the hipEvent time of all kernels of
 * the call. */
int gsa_align_pair_semi_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                            const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                            int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                            int64_t* cigar_need, gsa_align_pair_semi_info* info, float* kernel_ms, void* stream);

/* Long pairs, semi-global: scores and alignments of a batch in one call.
 *
 * gsa_score_semi_batch_dev takes gsa_score_batch_dev's arguments without local: pairs is a HOST array
 * (only seqY -- the query --, adjrows, seqX -- the subject --, and adjcols are read; two entries may
 * name the same buffers), out a host array of npairs results.  Synchronous.
 * Semantics: out[p] is exactly what gsa_score_semi_dev returns for pair p alone, with calc_kernel_ms
 * 0, whatever the pair's position or neighbours in the list; *batch_kernel_ms (may be null) gets the
 * hipEvent time of the launch.  Pairs with an empty side are answered on the host as there.
 * How: the batched semi-global instances of the K-rows score kernel (nw_kscore_semi_batch.hip) run all
 * pairs' tickets in one launch, 4 rows per lane in both gap models (GSA_SCORE_K=2 forces 2), the int8
 * profile for linear gaps only (GSA_KROW_Q8 = 0 / 2: int16 / int8 always), as gsa_score_batch_dev
 * chooses them.  Every pair's row R goes to its own part of one row buffer, 4 (C + 208) bytes rounded
 * up to 64, one workgroup per pair takes its first maximum, and one copy brings all answers back.
 * Memory: the checkpoint rows the launch keeps cost 16 bytes per subject column per ticket (of 256 K
 * rows) per pair; so callers pass subject windows, not chromosomes.  A batch whose rows cannot be
 * allocated returns the allocation error with nothing launched.  All scratch is counted in
 * gsa_mem_stats.
 * The mode has no second path, so no pair is routed elsewhere: it is errorInvalidValue, before
 * anything is enqueued, for everything gsa_score_batch_dev rejects and when any one pair is a pair
 * gsa_score_semi_dev refuses (its four conditions); out is then left as it was, the entries of the
 * pairs with an empty side included.  The call adds no launch kind and no knob, leaves the record of
 * gsa_last_launch and the fills' sticky error word alone, and reports kernel errors in the score
 * kernels' own control word.  An end column outside 0 ... C is errorKernelFailure. */
int gsa_score_semi_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                             int32_t substsz, int32_t gapo, int32_t gape, gsa_score_result* out,
                             float* batch_kernel_ms, void* stream);

typedef struct gsa_align_batch_semi_info {  /* what the call ran; optional out-parameter */
    int32_t batch_pairs;    /* pairs traced on the device */
    int32_t host_pairs;     /* pairs answered on the host: an empty side, an end cell on column 0 */
    int32_t strip_rows;     /* TR: rows of a strip, the batched score kernel's ticket (1024; 512 with
                               GSA_SCORE_K=2); 0: that kernel did not run */
    int32_t strips;         /* strips that hold the rows 1 ... R, over all traced pairs */
    int32_t strips_filled;  /* strips filled with move codes, over all rounds */
    int32_t rounds;         /* fill + walk launch pairs */
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    int64_t window_cols;    /* sum over the traced pairs of j_end - jW */
    int64_t gran_bytes;     /* bytes of checkpoint rows the score launch kept */
    float score_ms, fill_ms, walk_ms; /* hipEvent time of the batched score launch, and of the fill and the walk
                                         launches summed over the rounds */
    int32_t pad0;
} gsa_align_batch_semi_info;

/* The semi-global alignments of npairs pairs traced on the device together: gsa_align_batch_dev's
 * arguments without local.  Synchronous.
 * Semantics: out[p] is, field for field, what gsa_align_pair_semi_dev returns for pair p alone --
 * score, both cells and the CIGAR, the same recurrences, tie rule and stop in row 0 -- whatever the
 * strip height, the round, the pair's position or neighbours in the list and max_workgroups.  The
 * CIGAR buffer follows gsa_align_db_dev's rules as gsa_align_batch_dev states them: the strings back to
 * back in pair order, NUL-terminated, a pair's offset independent of cigar_cap, status 2 for a string
 * that does not fit, *cigar_need (may be null) the bytes all need.  Pairs with an empty side, and pairs
 * whose end cell is on column 0 (R x 'I'), are answered on the host as the single call answers them.
 * How: gsa_score_semi_batch_dev's launch leaves, per pair, the bottom row of each ticket of TR rows in
 * the pair's own hand-off rows; TR is 1024 (512 with GSA_SCORE_K=2), where gsa_align_pair_semi_dev
 * uses 512 for affine gaps.  Each pair gets its window jW from its own score and end column by that
 * call's formula with R its own query length; a strip's codes take (j_end - jW) TR / 2 bytes.  The
 * strips of many pairs are filled in one launch, one wave per strip, and the walks run side by side,
 * one wave per pair (nw_pair_semi_trace_batch.hip).  scratch_limit is the bytes of codes the call may
 * hold at once; 0 is the default, 8 GiB.  When the strips do not all fit the call runs rounds: the
 * pairs are taken by remaining code bytes descending, ties by index; each gets its lowest unfilled
 * strip and as many above it as still fit the round, for the columns jW + 1 ... j where its walk
 * stands; a pair for which nothing is left waits.  Every strip up to strip 0 is filled.  A round is one
 * upload of its tables, one fill launch, one walk launch and one small copy back.  max_workgroups caps
 * the grid of the fill and of the walk (0: all resident).
 * Memory: gsa_score_semi_batch_dev's rule -- 16 bytes of checkpoint rows per subject column per ticket
 * per pair (info.gran_bytes), so callers pass subject windows, not chromosomes; a batch whose rows
 * cannot be allocated returns the allocation error with nothing launched.  All scratch is counted in
 * gsa_mem_stats.
 * Status 1 -- score and end cell valid, start cell 0, an empty CIGAR -- for a pair one strip of whose
 * windowed codes exceeds scratch_limit.  The single call answers errorInvalidValue behind the score
 * launch there; a batch must not lose every answer to one pair, so here the other pairs are
 * unaffected.  The condition can differ from the single call's only through the strip height (1024
 * here against 512 there for affine gaps), at a limit between the two strip sizes.
 * The mode has no second path, so no pair is routed elsewhere: it is errorInvalidValue, before
 * anything is enqueued, for everything gsa_score_semi_batch_dev rejects, for any one pair that
 * gsa_align_pair_semi_dev would refuse (its value bound B of 2^26 or more included), for a negative
 * scratch_limit, cigar_cap or max_workgroups, a null out, or a null cigar with cigar_cap > 0.  A record
 * that comes back out of range, or a walk that left its window, is errorKernelFailure.  *info (may be
 * null) says what the call ran.  The call adds no launch kind and no knob and leaves the record of
 * gsa_last_launch and the fills' sticky error word alone.  *kernel_ms (may be null) gets the hipEvent
 * time of all kernels of the call. */
int gsa_align_batch_semi_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                             int32_t substsz, int32_t gapo, int32_t gape, int32_t max_workgroups,
                             int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                             int64_t* cigar_need, gsa_align_batch_semi_info* info, float* kernel_ms, void* stream);

/* Long pairs, overlap (dovetail) mode: score and alignment of one pair.
 * The suffix of one sequence against the prefix of the other (assembly, read merging, a read hanging
 * over the end of a contig), or either sequence within the other.  seqY has R letters and runs down the
 * rows, seqX has C letters and runs along the columns, both with the header element in front;
 * gapo <= gape <= 0.
 *   row 0 is free:     H(0, j) = 0, E = F = minus infinity, j = 0 ... C;
 *   column 0 is free:  H(i, 0) = 0, E = F = minus infinity, i = 0 ... R;
 *   inside, the Gotoh recurrences without the zero floor;
 *   the candidates are the cells of row R (j = 0 ... C) and of column C (i = 0 ... R); score is the
 *   largest H among them, so score >= 0 always;
 *   end cell: if a cell of row R attains the score, (R, SMALLEST such j) -- gsa_score_semi_dev's rule on
 *   that row --; otherwise (SMALLEST such i, C).  A score of 0 therefore always ends at (R, 0).
 * The walk starts at the end cell in state H and follows gsa_align_db_dev's rules -- diagonal before F
 * before E at equal value, a gap extended only when that is strictly better than opening -- and stops
 * as soon as i = 0 or j = 0; (i_start, j_start) is the cell where it stopped.  No gap letters are
 * emitted along either border, so all four overhangs stay out of the CIGAR; its letters are = X I D as
 * elsewhere.  Score 0: cells (R, 0)-(R, 0), an empty CIGAR, status 0, no fill launched (chunks = 0).
 * R = 0 or C = 0: score 0 with the cells that rule gives, (R, 0)-(R, 0), answered on the host.
 * The one call covers all four arrangements: X's suffix on Y's prefix, Y's suffix on X's prefix, Y
 * inside X, X inside Y.
 *
 * gsa_score_overlap_dev takes gsa_score_semi_dev's arguments and fills the same result struct.
 * Synchronous.  The pair runs in one direction on the K-rows score kernel's overlap instances
 * (nw_kscore_overlap.hip), the semi-global instances with two additions that live in a few blocks of a
 * strip: the floor H = 0 at the one step a lane stands on column 0, and column C of every row, which
 * every strip of every ticket stores once into a column buffer of 4 (1 + TR ceil(R / TR)) bytes in
 * the context's scratch (counted in gsa_mem_stats) next to the semi-global row buffer.  A small kernel
 * behind the fill takes the maximum over row R, column C and the analytic H(R, 0) = H(0, C) = 0 under
 * the tie rule above, and one copy brings score and end cell back.  GSA_SCORE_K and GSA_KROW_Q8 are
 * honoured as in gsa_score_semi_dev and no other knob is read.
 * The mode has no second path.  It is errorInvalidValue, before anything is enqueued, for everything
 * gsa_score_semi_dev refuses, under the same four conditions on B, the span, the LDS and the int16
 * table window.  The call adds no launch kind and no knob: the record of gsa_last_launch is left
 * untouched, and the kernel reports errors in the score kernels' own control word. */
int gsa_score_overlap_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                          const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                          gsa_score_result* out, void* stream);

typedef struct gsa_align_pair_overlap_info {  /* what the call ran; optional out-parameter */
    int32_t strip_rows;     /* TR: rows of a strip, the score kernel's ticket (512 or 1024) */
    int32_t strips;         /* strips that hold the rows 1 ... i_end */
    int32_t strips_filled;  /* strips filled with move codes, over all chunks */
    int32_t chunks;         /* fill + walk launch pairs */
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    float score_ms, fill_ms, walk_ms; /* hipEvent time of the score launch, and of the fill and the walk launches
                                         summed over the chunks */
    int32_t pad0;
} gsa_align_pair_overlap_info;

/* The overlap alignment of one long pair, traced on the device: gsa_align_pair_semi_dev's arguments,
 * result struct and CIGAR buffer rules (one NUL-terminated string at cigar[0], status 2 when it does
 * not fit cigar_cap with the cells still valid, *cigar_need the bytes it needs, 2 (R + C) + 1 always
 * enough).  Synchronous.  Score, end cell, walk and start cell are as stated above.
 * How: gsa_score_overlap_dev's launch leaves the bottom row of each of its tickets of TR rows (512,
 * linear gaps 1024) in its hand-off rows.  The strips from the one that holds i_end upwards are
 * refilled with 4-bit move codes over the columns 1 ... j_end, one wave per strip, under the borders
 * above (nw_pair_overlap_trace.hip), and one lane walks the codes; an end cell on column C above row R
 * leaves the strips below it alone.  A strip's codes take j_end TR / 2 bytes: codes run from column 1,
 * there is no column window.  scratch_limit is the bytes of codes the call may hold at once; 0 is the
 * default, 2 GiB.  The strips are taken bottom-up in chunks of consecutive strips that fit, a fill and
 * a walk launch and one small copy back per chunk; a later chunk is filled only up to the column where
 * the walk left the one below, and the strips above the chunk in which the walk reached column 0 are
 * not filled at all.  The scratch is counted in the peaks of gsa_mem_stats.
 * No result has status 1.  The call is errorInvalidValue, before anything is enqueued, for everything
 * gsa_score_overlap_dev refuses, for a pair whose value bound B reaches 2^26 (the fill keeps 4 x value
 * + source), for a negative scratch_limit or cigar_cap, a null out or a null cigar with cigar_cap > 0;
 * and errorInvalidValue behind the score launch, which alone knows j_end, for a scratch_limit below one
 * strip's codes.  *info (may be null) says what the call ran.  The call adds no launch kind and no knob
 * and leaves the record of gsa_last_launch and the fills' sticky error word alone.  *kernel_ms (may be
 * null) gets the hipEvent time of all kernels of the call. */
int gsa_align_pair_overlap_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                               const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape,
                               int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                               int64_t* cigar_need, gsa_align_pair_overlap_info* info, float* kernel_ms, void* stream);

/* Long pairs, overlap (dovetail) mode: scores and alignments of a batch in one call.
 *
 * gsa_score_overlap_batch_dev takes gsa_score_semi_batch_dev's arguments: pairs is a HOST array (only
 * seqY, adjrows, seqX and adjcols are read; two entries may name the same buffers), out a host array
 * of npairs results.  Synchronous.
 * Semantics: out[p] is exactly what gsa_score_overlap_dev returns for pair p alone, with calc_kernel_ms
 * 0, whatever the pair's position or neighbours in the list, the rows per lane and the profile width;
 * *batch_kernel_ms (may be null) gets the hipEvent time of the launch.  Pairs with an empty side are
 * answered on the host as there: score 0 at (R, 0).
 * How: the batched overlap instances of the K-rows score kernel (nw_kscore_overlap_batch.hip) run all
 * pairs' tickets in one launch, 4 rows per lane in both gap models (GSA_SCORE_K=2 forces 2), the int8
 * profile for linear gaps only (GSA_KROW_Q8 = 0 / 2: int16 / int8 always), as gsa_score_semi_batch_dev
 * chooses them.  Every pair's row R goes to its own part of one row buffer, 4 (C + 208) bytes rounded
 * up to 64, and column C of every row of every one of its tickets to its own part of one column buffer,
 * 4 (1 + TR ceil(R / TR)) bytes rounded up to 64 -- the rows past R are stored too, so the pair's last
 * ticket counts whole.  One workgroup per pair takes the maximum over its row R, its column C and the
 * analytic H(R, 0) = H(0, C) = 0 under gsa_score_overlap_dev's tie rule, and one copy brings all
 * answers back.
 * Memory: the checkpoint rows the launch keeps cost 16 bytes per column per ticket (of 256 K rows) per
 * pair.  A batch whose buffers cannot be allocated returns the allocation error with nothing launched.
 * All scratch is counted in gsa_mem_stats.
 * The mode has no second path, so no pair is routed elsewhere: it is errorInvalidValue, before
 * anything is enqueued, for everything gsa_score_semi_batch_dev rejects and when any one pair is a pair
 * gsa_score_overlap_dev refuses (its four conditions); out is then left as it was.  The call adds no
 * launch kind and no knob, leaves the record of gsa_last_launch and the fills' sticky error word alone,
 * and reports kernel errors in the score kernels' own control word.  An end cell that lies neither on
 * row R nor on column C is errorKernelFailure. */
int gsa_score_overlap_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                                int32_t substsz, int32_t gapo, int32_t gape, gsa_score_result* out,
                                float* batch_kernel_ms, void* stream);

typedef struct gsa_align_batch_overlap_info {  /* what the call ran; optional out-parameter */
    int32_t batch_pairs;    /* pairs traced on the device */
    int32_t host_pairs;     /* pairs answered on the host: an empty side, or score 0 at (R, 0) */
    int32_t strip_rows;     /* TR: rows of a strip, the batched score kernel's ticket (1024; 512 with
                               GSA_SCORE_K=2); 0: that kernel did not run */
    int32_t strips;         /* strips that hold the rows 1 ... i_end, over the traced pairs */
    int32_t strips_filled;  /* strips filled with move codes, over all rounds; less than strips when a
                               walk reached column 0 below strip 0 */
    int32_t rounds;         /* fill + walk launch pairs */
    int64_t code_bytes;     /* peak bytes of move codes held at once */
    int64_t gran_bytes;     /* bytes of checkpoint rows the score launch kept */
    float score_ms, fill_ms, walk_ms; /* hipEvent time of the batched score launch, and of the fill and the walk
                                         launches summed over the rounds */
    int32_t pad0;
} gsa_align_batch_overlap_info;

/* The overlap alignments of npairs pairs traced on the device together: gsa_align_batch_semi_dev's
 * arguments.  Synchronous.
 * Semantics: out[p] is, field for field, what gsa_align_pair_overlap_dev returns for pair p alone --
 * score, both cells and the CIGAR, the same recurrences, tie rules and stop on either free border --
 * whatever the strip height, the round, the pair's position or neighbours in the list and
 * max_workgroups.  The CIGAR buffer follows gsa_align_db_dev's rules as gsa_align_batch_dev states
 * them: the strings back to back in pair order, NUL-terminated, a pair's offset independent of
 * cigar_cap, status 2 for a string that does not fit, *cigar_need (may be null) the bytes all need.
 * Pairs with an empty side, and pairs whose score is 0 at (R, 0), are answered on the host as the
 * single call answers them: the cells (R, 0)-(R, 0) and an empty CIGAR.
 * How: gsa_score_overlap_batch_dev's launch leaves, per pair, the bottom row of each ticket of TR rows
 * in the pair's own hand-off rows; TR is 1024 (512 with GSA_SCORE_K=2), where gsa_align_pair_overlap_dev
 * uses 512 for affine gaps.  A pair's strips run from the one that holds its i_end upwards -- an end
 * cell on column C above row R leaves the strips below it alone -- and a strip's codes take
 * j_end TR / 2 bytes: codes run from column 1, there is no column window.  The strips of many pairs are
 * filled in one launch, one wave per strip, and the walks run side by side, one wave per pair
 * (nw_pair_overlap_trace_batch.hip).  scratch_limit is the bytes of codes the call may hold at once; 0
 * is the default, 8 GiB.  When the strips do not all fit the call runs rounds: the pairs are taken by
 * remaining code bytes descending, ties by index; each gets its lowest unfilled strip and as many above
 * it as still fit the round, for the columns 1 ... j where its walk stands; a pair for which nothing is
 * left waits.  A pair whose walk stands on row 0 or on column 0 after a round is done, and the strips
 * above the chunk in which it reached column 0 are not filled at all (info.strips_filled <
 * info.strips).  A round is one upload of its tables, one fill launch, one walk launch and one small
 * copy back.  max_workgroups caps the grid of the fill and of the walk (0: all resident).
 * Memory: gsa_score_overlap_batch_dev's rule (info.gran_bytes); all scratch is counted in
 * gsa_mem_stats.
 * Status 1 -- score and end cell valid, start cell 0, an empty CIGAR -- for a pair one strip of whose
 * codes (j_end TR / 2 bytes) exceeds scratch_limit.  The single call answers errorInvalidValue behind
 * the score launch there; a batch must not lose every answer to one pair, so here the other pairs are
 * unaffected.  The condition can differ from the single call's only through the strip height (1024
 * here against 512 there for affine gaps), at a limit between the two strip sizes.
 * The mode has no second path, so no pair is routed elsewhere: it is errorInvalidValue, before
 * anything is enqueued, for everything gsa_score_overlap_batch_dev rejects, for any one pair that
 * gsa_align_pair_overlap_dev would refuse (its value bound B of 2^26 or more included), for a negative
 * scratch_limit, cigar_cap or max_workgroups, a null out, or a null cigar with cigar_cap > 0; out is
 * then left as it was.  A record that comes back out of range, or a walk that stopped neither on a
 * free border nor on its chunk's upper boundary, is errorKernelFailure.  *info (may be null) says what
 * the call ran.  The call adds no launch kind and no knob and leaves the record of gsa_last_launch and
 * the fills' sticky error word alone.  *kernel_ms (may be null) gets the hipEvent time of all kernels
 * of the call. */
int gsa_align_batch_overlap_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                                int32_t substsz, int32_t gapo, int32_t gape, int32_t max_workgroups,
                                int64_t scratch_limit, gsa_align_db_result* out, char* cigar, int64_t cigar_cap,
                                int64_t* cigar_need, gsa_align_batch_overlap_info* info, float* kernel_ms, void* stream);

/* Long pairs, banded: score and alignment of one pair inside a diagonal band.
 * For two related long sequences -- two assemblies of one locus, a corrected read against its
 * reference window, two haplotypes -- almost all of the R x C rectangle cannot hold the alignment.
 * These two calls fill a band of diagonals only, and write the move codes in the same pass.
 *
 * Semantics.  seqY is the query, R letters, down the rows.  seqX is the subject, C letters, along the
 * columns.  Both carry the header element in front.  gapo <= gape <= 0.
 * The band is a pair band_lo <= band_hi of diagonals j - i.  Cell (i, j), 0 <= i <= R, 0 <= j <= C, is
 * in the band iff band_lo <= j - i <= band_hi.
 *   Every cell outside the band has H = E = F = minus infinity, border cells included.
 *   Inside the band: gsa_align_pair_dev's global recurrences, borders, tie rule and CIGAR letters.
 *     H(0, 0) = 0.
 *     Row 0: H = E = go + (j - 1) ge, F = minus infinity.
 *     Column 0: H = F = go + (i - 1) ge, E = minus infinity.
 *     Walk from (R, C) in state H: diagonal before F before E.
 *     A gap is extended only when that is strictly better than opening.
 *     Row 0 is E only, column 0 is F only.
 *   Results: score = H(R, C); end cell (R, C), start cell (0, 0); the CIGAR of that walk, which by
 *   construction never leaves the band.
 *   Validity: band_lo <= min(0, C - R) and band_hi >= max(0, C - R), else errorInvalidValue, since no
 *   alignment exists.  The call clamps band_lo to -R and band_hi to C.  Wider changes nothing.  The
 *   info struct reports the clamped values.
 *   W = band_hi - band_lo + 1 after clamping must be at most a compile-time limit, which
 *   gsa_band_max_width() returns (5826: nw_band_plan.h derives it from the waves' schedule).  Beyond
 *   it the call is errorInvalidValue: the unbanded calls are the tool for bands that wide.
 *   R = 0 or C = 0 are answered on the host: all-D or all-I, under the same validity rule and
 *   gsa_score_dev's value range for the one gap run (the width limit does not apply there: nothing is
 *   launched).
 *   Minus infinity is any finite value that never wins.  Every in-band cell is reachable from (0, 0)
 *   inside the band, so a real H exists at every in-band cell.  E / F values derived from minus
 *   infinity are one step deep and never accumulate.
 * The certificate (proved_optimal).  Let pmax = max(0, largest table value), D = C - R, S the banded
 * score, and band_lo, band_hi the clamped values.
 *   A path that leaves the band on the high side has at least band_hi + 1 letters of D and
 *   band_hi + 1 - D of I.  So it scores at most
 *     U_hi = pmax (C - band_hi - 1) + 2 gapo + band_hi gape + (band_hi - D) gape.
 *   This applies only if band_hi < C.
 *   On the low side, with a = 1 - band_lo, a path scores at most
 *     U_lo = pmax (R - a) + 2 gapo + (a - 1) gape + (a + D - 1) gape.
 *   This applies only if band_lo > -R.
 *   proved_optimal = 1 iff S is strictly greater than every bound that applies.
 *   Then every optimal unbanded alignment lies in the band, and the call's six fields and CIGAR are
 *   exactly those of gsa_align_pair_dev for the same pair (global).  Strictness is what makes ties safe.
 *
 * How (nw_band.hip): one workgroup of min(16, strips) waves.  Strip s holds the rows s TR + 1 ...
 * (s + 1) TR (TR = 256, 4 rows per lane) and sweeps only the W + TR - 1 columns from its own origin
 * s TR + 1 + band_lo.  The waves run in lockstep super-steps of 64 columns with one workgroup barrier
 * between them; strip s starts at super-step 6 s on wave s mod 16 and takes the row above it from a
 * ring in LDS that strip s - 1 filled in strictly earlier super-steps.  Nothing polls memory.  The
 * alignment call stores the 4-bit move codes of the band in that one pass, strips x (W + TR - 1) x
 * TR / 2 bytes in all, and one lane walks them; there are no checkpoint rows, no refill and no chunks.
 * One workgroup is a sliver of the chip: the calls pay when the band is a small part of the
 * rectangle (DESIGN.md 2.2p has the measurements).
 *
 * Both calls are synchronous.  gsa_score_band_dev fills gsa_score_dev's result struct: score, end
 * cell (R, C), the hipEvent time of the fill.  It runs the instance without move codes, on plain
 * int32 values.  Refusals, all errorInvalidValue before anything is enqueued: everything gsa_score_dev
 * rejects for a global pair, B + |gapo| < 2^29 included, with B = smax min(R, C) + |gapo| +
 * (R + C) |gape| (inside the band every cell is reached by one gap and a diagonal run, so the same
 * bound holds); R or C of 2^30 or more; the validity and width rules above; a null out.  The calls
 * add no launch kind and no knob, leave the record of gsa_last_launch and the fills' sticky error
 * word alone, and count their scratch in gsa_mem_stats. */
int64_t gsa_band_max_width(void);
int gsa_score_band_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                       const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo,
                       int64_t band_hi, gsa_score_result* out, void* stream);

typedef struct gsa_align_pair_band_info {  /* what the call ran; optional out-parameter */
    int32_t strip_rows;      /* TR: rows of a strip (256) */
    int32_t strips;          /* strips that hold the rows 1 ... R */
    int32_t waves;           /* waves of the workgroup */
    int32_t supersteps;      /* T: barriers of the workgroup, (strips - 1) lag + ceil((W + TR + 62) / 64) */
    int32_t proved_optimal;  /* the certificate above */
    int32_t pad0;
    int64_t band_lo, band_hi; /* the clamped band */
    int64_t code_bytes;      /* bytes of move codes of the band (also when they exceed scratch_limit) */
    float score_ms, walk_ms; /* hipEvent time of the fill and of the walk */
} gsa_align_pair_band_info;

/* The banded alignment of one long pair, traced on the device: gsa_score_band_dev's arguments,
 * gsa_align_pair_dev's result struct and CIGAR buffer rules (one NUL-terminated string at cigar[0],
 * status 2 when it does not fit cigar_cap with the cells still valid, *cigar_need the bytes it needs,
 * 2 (R + C) + 1 always enough).  scratch_limit is the bytes of move codes the call may hold; 0 is the
 * default, 2 GiB.  Status 1 means score and end cell from the instance without codes and an empty
 * CIGAR; it applies when B reaches 2^26 (the fill keeps 4 x value + source) or when code_bytes
 * exceeds scratch_limit (info->code_bytes says what it would take).  The walk's record is validated
 * on the host: at most R + C moves, ended at (0, 0); a step onto a cell outside the band is
 * errorKernelFailure.  errorInvalidValue, before anything is enqueued, for everything
 * gsa_score_band_dev refuses, a negative scratch_limit or cigar_cap and a null cigar with
 * cigar_cap > 0.  *info (may be null) says what the call ran; *kernel_ms (may be null) gets the
 * hipEvent time of both kernels. */
int gsa_align_pair_band_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                            const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo,
                            int64_t band_hi, int64_t scratch_limit, gsa_align_db_result* out, char* cigar,
                            int64_t cigar_cap, int64_t* cigar_need, gsa_align_pair_band_info* info, float* kernel_ms,
                            void* stream);

/* Long pairs, banded: scores and alignments of a batch in one call.
 *
 * gsa_score_band_batch_dev: pairs is a HOST array (only seqY, adjrows, seqX and adjcols are read; two
 * entries may name the same buffers), band_lo and band_hi host arrays with pair p's band at [p], out a
 * host array of npairs results.  Synchronous.
 * Semantics: out[p] is exactly what gsa_score_band_dev returns for pair p alone with band_lo[p],
 * band_hi[p], with calc_kernel_ms 0, whatever the pair's position or neighbours in the list, the waves
 * per workgroup and max_workgroups; *batch_kernel_ms (may be null) gets the hipEvent time of the
 * launch.  Pairs with R = 0 or C = 0 are answered on the host as there.
 * How (nw_band_batch.hip): one launch of the fill without move codes on a persistent grid of
 * min(pairs, resident workgroups, max_workgroups) workgroups (max_workgroups 0: no cap).  A workgroup
 * claims the next pair from one counter and runs gsa_score_band_dev's lockstep super-steps for it, the
 * same device code, then claims again; the pairs are handed out by super-steps T descending, ties by
 * index, so the longest start first.  Nothing polls memory and no workgroup waits for another.
 * waves is the waves per workgroup: 4, 8 or 16, or 0 for the smallest of the three on which every pair
 * of the launch with more strips than waves finds its wave free again, nq <= 6 waves with nq =
 * ceil((W + TR + 62) / 64), that is W <= 1218 at 4 waves, 2754 at 8 and 5826 at 16.  It is an argument
 * and no knob: no result depends on it.
 * errorInvalidValue, before anything is enqueued and with out left as it was: npairs < 0, a null array,
 * any one pair that gsa_score_band_dev refuses (an invalid band, a width over gsa_band_max_width(), the
 * value range), a negative max_workgroups, a waves that is none of 0, 4, 8, 16 or that is too small
 * for one of the pairs (more strips than waves and nq > 6 waves).  npairs = 0 succeeds with nothing
 * launched.  The call adds no launch kind and no knob, leaves the record of gsa_last_launch and the
 * fills' sticky error word alone, and counts its scratch in gsa_mem_stats. */
int gsa_score_band_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                             int32_t substsz, int32_t gapo, int32_t gape, const int64_t* band_lo,
                             const int64_t* band_hi, int32_t waves, int32_t max_workgroups, gsa_score_result* out,
                             float* batch_kernel_ms, void* stream);

typedef struct gsa_align_batch_band_pair {  /* one pair of the batch: gsa_align_pair_band_info's values */
    int64_t band_lo, band_hi; /* the clamped band */
    int64_t code_bytes;       /* bytes of move codes of the pair's band (also when it got none) */
    int32_t strips;           /* strips that hold the rows 1 ... R (0: answered on the host) */
    int32_t supersteps;       /* T of the pair */
    int32_t proved_optimal;   /* the certificate of gsa_align_pair_band_dev */
    int32_t round;            /* >= 0: the fill + walk round the pair ran in; -1: answered on the host;
                                 -2: it ran without codes (status 1) */
} gsa_align_batch_band_pair;

typedef struct gsa_align_batch_band_info {  /* what the call ran; optional out-parameter */
    int32_t batch_pairs;   /* pairs traced on the device */
    int32_t host_pairs;    /* pairs answered on the host: an empty side */
    int32_t nocode_pairs;  /* pairs that ran without codes: status 1 */
    int32_t rounds;        /* fill + walk launch pairs */
    int32_t waves;         /* waves per workgroup the launches used (the largest, when they differ) */
    int32_t strip_rows;    /* TR: rows of a strip (256); 0: nothing was launched */
    int64_t code_bytes;    /* peak bytes of move codes held at once */
    float fill_ms, nocode_ms, walk_ms; /* hipEvent time of the fills with codes, of the launch without and of
                                          the walks, summed over the rounds */
    int32_t pad0;
} gsa_align_batch_band_info;

/* The banded alignments of npairs pairs traced on the device together: gsa_score_band_batch_dev's
 * arguments, gsa_align_batch_dev's result array and CIGAR buffer.  Synchronous.
 * Semantics: out[p] is, field for field, what gsa_align_pair_band_dev returns for pair p alone with
 * band_lo[p], band_hi[p] -- score, both cells, status and the CIGAR -- whatever the pair's position or
 * neighbours in the list, the waves per workgroup, max_workgroups, the round it lands in, or whether two
 * entries name the same buffers.  pair_info[p] (a host array of npairs entries, may be null) holds the
 * single call's info values of pair p and its round.  The CIGAR buffer follows gsa_align_batch_dev's
 * rules: the strings back to back in pair order, NUL-terminated, a pair's offset independent of
 * cigar_cap, status 2 for a string that does not fit, *cigar_need (may be null) the bytes all need.
 * How: a pair's move codes are held whole, strips x (W + TR - 1) x TR / 2 bytes.  scratch_limit is the
 * bytes of codes the call may hold at once; 0 is the default, 8 GiB.  The pairs that get codes are taken
 * by code bytes descending, ties by index; a round takes every pair that still fits the bytes left,
 * first fit in that order, and is one upload of its descriptors, one fill launch on the persistent grid
 * above with the 4-bit codes written in the same pass, one walk launch -- one wave per pair, lane 0
 * walking as in the single call, workgroups taking the pairs b, b + grid, ... under max_workgroups --
 * and one copy that brings all records and move bytes of the round back.  A launch takes its waves
 * from its widest pair.
 * Status 1 -- score and end cell from the fill without codes, start cell 0, an empty CIGAR -- for a pair
 * whose own code_bytes exceed scratch_limit or whose value bound B reaches 2^26: the single call's
 * rule, with the batch's limit.  These pairs run in one launch without codes before the rounds; the
 * other pairs are unaffected.
 * errorInvalidValue, before anything is enqueued and with out left as it was: everything
 * gsa_score_band_batch_dev refuses, a negative scratch_limit or cigar_cap, a null cigar with
 * cigar_cap > 0.  A walk record that comes back out of range, or a step off the band, is
 * errorKernelFailure.  *info (may be null) says what the call ran; *kernel_ms (may be null) gets the
 * hipEvent time of all kernels of the call.  All scratch is counted in gsa_mem_stats; the record of
 * gsa_last_launch and the fills' sticky error word are left alone. */
int gsa_align_batch_band_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                             int32_t substsz, int32_t gapo, int32_t gape, const int64_t* band_lo,
                             const int64_t* band_hi, int32_t waves, int32_t max_workgroups, int64_t scratch_limit,
                             gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                             gsa_align_batch_band_pair* pair_info, gsa_align_batch_band_info* info, float* kernel_ms,
                             void* stream);

/* Long pairs, banded extension: the start fixed at (0, 0), the end free -- the best cell of the band; one
 * pair and a batch.  The step every seed-and-extend pipeline runs behind its outermost
 * anchor: the global banded call would drag the unrelated tails into the CIGAR, the local mode would
 * lose the anchor.  (Left extension: the caller reverses both sequences.)
 *
 * Semantics.  seqY, seqX, the table and gapo <= gape <= 0 as gsa_score_band_dev takes them.
 * The band is a pair band_lo <= band_hi of diagonals j - i.  Cell (i, j), 0 <= i <= R, 0 <= j <= C, is
 * in the band iff band_lo <= j - i <= band_hi; outside the band H = E = F = minus infinity.
 *   Values: exactly gsa_align_pair_band_dev's.  H(0, 0) = 0, row 0 is E only, column 0 is F only, the
 *   Gotoh recurrences inside.
 *   Validity: the band must hold (0, 0): band_lo <= 0 <= band_hi, else errorInvalidValue.  It need not
 *   hold (R, C).  The call clamps band_lo to -R and band_hi to C; the width after clamping must be at
 *   most gsa_band_max_width().
 *   Score: the maximum of H over all cells of the band.  It is never negative, since H(0, 0) = 0.
 *   End cell: the first maximal cell in row-major order (smallest i, then smallest j), the local
 *   mode's rule.  A score of 0 therefore ends at (0, 0) with an empty CIGAR and status 0; border cells
 *   other than (0, 0) never win.
 *   Alignment: the start cell is (0, 0).  Walk from the end cell in state H: diagonal before F before
 *   E; a gap is extended only when that is strictly better than opening.  CIGAR letters = X I D; the
 *   CIGAR consumes exactly i_end letters of seqY and j_end letters of seqX.
 *   R = 0 or C = 0 is answered on the host: score 0, end (0, 0), an empty CIGAR, status 0,
 *   proved_optimal 1.
 * Trimming.  Rows beyond C - band_lo and columns beyond R + band_hi hold no cell of the band.  The call
 * plans, launches and guards its value ranges on R' = min(R, C - band_lo), C' = min(C, R + band_hi)
 * (clamped band), and reports them as rows_used and cols_used; the result is that of the whole pair.
 * The certificate (proved_optimal).  Let pmax = max(0, largest table value), S the banded score, and
 * band_lo, band_hi the clamped values.
 *   A path that leaves the band on the high side holds at least band_hi + 1 letters of D.  No cell of
 *   it behind that scores more than
 *     U_hi = pmax min(R, C - band_hi - 1) + gapo + band_hi gape.
 *   This applies only if band_hi < C.
 *   On the low side, with a = 1 - band_lo,
 *     U_lo = pmax min(C, R - a) + gapo + (a - 1) gape.
 *   This applies only if band_lo > -R.
 *   proved_optimal = 1 iff S is strictly greater than every bound that applies.
 *   Then the score, both cells and the CIGAR are those of the unbanded extension (the band -R ... C).
 *
 * How (nw_band_ext.hip, nw_band_ext_batch.hip): gsa_score_band_dev's workgroup, strips, super-steps and
 * ring, the same device body with one addition.  Every lane keeps the best value and its column for
 * each of its 4 rows (one compare and two selects per cell), folds them at the end of a strip, and
 * behind the last super-step the lanes reduce by shuffles, the waves through one LDS slot each behind
 * one barrier.  Nothing polls memory and the reduction uses no atomics.  The fill writes score and end
 * cell into its result words, and the walk -- enqueued behind it -- starts where they say.
 *
 * gsa_score_band_ext_dev fills gsa_score_dev's result struct: score, end cell, the hipEvent time of the
 * fill.  Refusals, all errorInvalidValue before anything is enqueued: everything gsa_score_band_dev
 * refuses, with its validity rule replaced by the one above and the value range B taken on (R', C').
 * Not here: X-drop or Z-drop termination, the best score at the query's end, left extension.  The
 * calls add no launch kind and no knob, leave the record of gsa_last_launch and the fills' sticky error
 * word alone, and count their scratch (the global banded calls' buffers) in gsa_mem_stats. */
int gsa_score_band_ext_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                           const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo,
                           int64_t band_hi, gsa_score_result* out, void* stream);

typedef struct gsa_align_pair_band_ext_info {  /* gsa_align_pair_band_info's fields, of the trimmed pair */
    int32_t strip_rows;      /* TR: rows of a strip (256) */
    int32_t strips;          /* strips that hold the rows 1 ... R' */
    int32_t waves;           /* waves of the workgroup */
    int32_t supersteps;      /* T: barriers of the workgroup */
    int32_t proved_optimal;  /* the certificate above */
    int32_t pad0;
    int64_t band_lo, band_hi; /* the clamped band */
    int64_t code_bytes;      /* bytes of move codes of the band (also when they exceed scratch_limit) */
    float score_ms, walk_ms; /* hipEvent time of the fill and of the walk */
    int64_t rows_used, cols_used; /* R', C': the part of the pair the band reaches */
} gsa_align_pair_band_ext_info;

/* The banded extension alignment of one long pair, traced on the device: gsa_align_pair_band_dev's
 * arguments, buffers and rules for scratch_limit, cigar_cap, cigar_need and status.  Status 1 (no codes
 * were kept: B on (R', C') reaches 2^26, or code_bytes exceeds scratch_limit): score and end cell are
 * still returned, the CIGAR is empty.  Status 2: the CIGAR does not fit.  The walk's record is
 * validated on the host: not off the band, ended at (0, 0), at most i_end + j_end moves; the end cell
 * inside the trimmed matrix and inside the band; else errorKernelFailure. */
int gsa_align_pair_band_ext_dev(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
                                const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int64_t band_lo,
                                int64_t band_hi, int64_t scratch_limit, gsa_align_db_result* out, char* cigar,
                                int64_t cigar_cap, int64_t* cigar_need, gsa_align_pair_band_ext_info* info,
                                float* kernel_ms, void* stream);

/* The scores of a batch: gsa_score_band_batch_dev's arguments, persistent grid, waves rule and refusals.
 * out[p] is exactly what gsa_score_band_ext_dev returns for pair p alone (calc_kernel_ms 0), whatever
 * its position, its neighbours, the waves or the grid. */
int gsa_score_band_ext_batch_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                                 int32_t substsz, int32_t gapo, int32_t gape, const int64_t* band_lo,
                                 const int64_t* band_hi, int32_t waves, int32_t max_workgroups, gsa_score_result* out,
                                 float* batch_kernel_ms, void* stream);

typedef struct gsa_align_batch_band_ext_pair {  /* one pair of the batch: gsa_align_pair_band_ext_info's values */
    int64_t band_lo, band_hi; /* the clamped band */
    int64_t code_bytes;       /* bytes of move codes of the pair's band (also when it got none) */
    int64_t rows_used, cols_used; /* R', C' of the pair */
    int32_t strips;           /* strips that hold the rows 1 ... R' (0: answered on the host) */
    int32_t supersteps;       /* T of the pair */
    int32_t proved_optimal;   /* the certificate of gsa_align_pair_band_ext_dev */
    int32_t round;            /* >= 0: the fill + walk round the pair ran in; -1: answered on the host;
                                 -2: it ran without codes (status 1) */
} gsa_align_batch_band_ext_pair;

typedef struct gsa_align_batch_band_ext_info {  /* gsa_align_batch_band_info's fields */
    int32_t batch_pairs;   /* pairs traced on the device */
    int32_t host_pairs;    /* pairs answered on the host: an empty side */
    int32_t nocode_pairs;  /* pairs that ran without codes: status 1 */
    int32_t rounds;        /* fill + walk launch pairs */
    int32_t waves;         /* waves per workgroup the launches used (the largest, when they differ) */
    int32_t strip_rows;    /* TR: rows of a strip (256); 0: nothing was launched */
    int64_t code_bytes;    /* peak bytes of move codes held at once */
    float fill_ms, nocode_ms, walk_ms; /* hipEvent time of the fills with codes, of the launch without and of
                                          the walks, summed over the rounds */
    int32_t pad0;
    int64_t rows_used, cols_used; /* R' and C' summed over the pairs that ran on the device */
} gsa_align_batch_band_ext_info;

/* The alignments of a batch: gsa_align_batch_band_dev's arguments, rounds, CIGAR buffer and refusals.
 * out[p] is, field for field, what gsa_align_pair_band_ext_dev returns for pair p alone, and
 * pair_info[p] its info values, whatever the pair's position, its neighbours, the waves, the grid or the
 * round.  Nothing is enqueued before every pair has passed its checks. */
int gsa_align_batch_band_ext_dev(gsa_ctx* ctx, int32_t npairs, const gsa_pair_dev* pairs, const int32_t* subst,
                                 int32_t substsz, int32_t gapo, int32_t gape, const int64_t* band_lo,
                                 const int64_t* band_hi, int32_t waves, int32_t max_workgroups, int64_t scratch_limit,
                                 gsa_align_db_result* out, char* cigar, int64_t cigar_cap, int64_t* cigar_need,
                                 gsa_align_batch_band_ext_pair* pair_info, gsa_align_batch_band_ext_info* info,
                                 float* kernel_ms, void* stream);

/* Host buffers (alloc, copy in, fill, laps as gsa_align_*). */
int gsa_score(gsa_ctx* ctx, const int32_t* seqY, int32_t adjrows, const int32_t* seqX, int32_t adjcols,
              const int32_t* subst, int32_t substsz, int32_t gapo, int32_t gape, int32_t local,
              gsa_score_result* out, gsa_laps* laps);

#ifdef __cplusplus
}
#endif

#endif /* GSA_H */
