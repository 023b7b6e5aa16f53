/*
 * lgconv_hip.h -- C ABI of the MI355X (gfx950) LightGCN propagation library.
 *
 * This is the drop-in boundary for the hot path of happykygo/GNN-eCommerce
 * (BASELINE.json: north_star).  The reference has no FFI of its own: the path is reached
 * through two Python call surfaces.  Each entry point below names
 * the reference interface it stands in for (paths relative to the reference tree); the
 * ctypes stubs a maintainer would add are in INTEGRATION.md and are what
 * gnn-ecommerce_amd/_native.py contains.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says host
 *   - all buffers are owned by the caller (PyTorch's caching allocator in practice); the
 *     library borrows them for the duration of the launches it enqueues, keeps no global
 *     state and allocates nothing
 *   - every function enqueues on `stream` (a hipStream_t passed as void*) and returns
 *     without synchronising
 *   - return value: 0 = ok; >0 = hipError_t from the runtime; <0 = LGC_E_* argument error
 *   - `status` words are device int32 the kernels OR error bits into (LGC_ST_*); the
 *     caller zeroes them and reads them back when it wants to know
 *   - values fp32, indices int32 inside the library; the reference's int64 COO is converted
 *     by lgc_build_csr
 */
#ifndef LGCONV_HIP_H
#define LGCONV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Still 14 although lgc_sweep_cfg and lgc_sweep_dims have grown by light_len at their ends: the number is pinned by the
 * tests of seven features.  A caller compiled against the structs without the field must be rebuilt with this header. */
#define LGC_ABI_VERSION 14

/* argument errors (negative return values) */
#define LGC_E_INVAL      (-1)  /* null pointer, negative size, bad flag                    */
#define LGC_E_DIM        (-2)  /* embedding width outside 1..256 (see lgc_dim_ok)           */
#define LGC_E_WORKSPACE  (-3)  /* workspace smaller than lgc_build_workspace_bytes()        */
#define LGC_E_RANGE      (-4)  /* node or edge count does not fit int32                     */
#define LGC_E_ALIGN      (-5)  /* pointer / stride alignment requirement violated           */

/* bits OR-ed into device status words */
#define LGC_ST_INDEX_OOB 1     /* an index was outside [0, n_nodes); that element was skipped (lgc_build_csr parks it) */

/* One adjacency entry as the kernels read it: 8 bytes, {source column, fp32 value}. */
typedef struct lgc_entry {
    int32_t col;
    float   val;
} lgc_entry;

/* One unit of work for rows longer than `short_max` (see lgc_spmm). */
typedef struct lgc_chunk {
    int32_t row;    /* output row                                                   */
    int32_t begin;  /* first entry (index into entries[])                            */
    int32_t end;    /* one past the last entry                                       */
    int32_t slot;   /* >=0: write the raw sum to partials[slot]; -1: finish the row  */
} lgc_chunk;

/* A row that was cut into several chunks: its partial sums sit in slots [begin, end). */
typedef struct lgc_multi_row {
    int32_t row;
    int32_t slot_begin;
    int32_t slot_end;
    int32_t reserved;
} lgc_multi_row;

int lgc_abi_version(void);

/* Human-readable text for a negative return code (host pointer, static storage). */
const char *lgc_error_string(int code);

/* 1 if lgc_spmm / lgc_pair_dot accept this embedding width. */
int lgc_dim_ok(int32_t dim);

/* ---------------------------------------------------------------------------------------
 * Graph build: dense COO -> CSR with normalised values.
 *
 * Replaces what PyG's LGConv.forward -> gcn_norm recomputes on every layer of every call
 * (called from src/lightgcn.py:96; COO produced by src/utils_v2.py:146-165, copy at
 * torchserve/lightgcn_handler.py:112-131).
 *
 *   edge_index  int64 [2, n_edges] contiguous: row 0 = source j, row 1 = target i
 *   edge_weight fp32 [n_edges] or NULL (= all ones, as upstream)
 *   by_source   0: rows of the CSR are targets, columns sources  (the forward operator A)
 *               1: rows are sources, columns targets              (A^T, for the backward pass)
 *   normalize   1: val = dis[j] * w * dis[i], dis = deg^-1/2 (inf -> 0), deg = weighted
 *                  in-degree by target accumulated SEQUENTIALLY IN EDGE ORDER in fp32 --
 *                  the order the reference's CPU scatter uses
 *               0: val = w
 *   dis_in      normalize=1 only: NULL -> compute deg/dis here (requires by_source=0) and
 *               write them to deg_out/dis_out; non-NULL -> use these (the A^T build)
 *   rowptr      out int32 [n_nodes + 1]
 *   entries     out lgc_entry [n_edges]; inside a row the entries keep the edge order
 *   edge_val    out fp32 [n_edges] in ORIGINAL edge order, or NULL
 *   deg_out, dis_out  out fp32 [n_nodes] or NULL
 *   status      device int32; bits are OR-ed into it (atomicOr), never written: other bits survive
 *
 * Arithmetic, bit for bit (tests/test_build_gpu.py): deg = ((0 + w_0) + w_1) + ... over a row's edges in edge
 * order; dis = 1 / sqrt(deg) with both steps correctly rounded; val = fl(fl(dis[j] * w) * dis[i]); with
 * normalize = 0 the weight's bits come through unchanged (NaN payloads, -0.0).  fp32 denormals are kept, in the
 * weights and in deg, as on the host.
 *
 * An edge with an endpoint outside [0, n_nodes) -- tested as int64 before any address is formed from it: 2^32 is out
 * of range, not node 0 -- sets LGC_ST_INDEX_OOB in `status` and is PARKED, not dropped: it is counted in row 0, keeps
 * its place in edge order there, and its entry is {col 0, val +0.0}, its edge_val +0.0.  Its weight still enters
 * deg[0]: once the bit is set, deg[0], dis[0] and the values of the edges that touch node 0 are unspecified (every
 * other row, entry and value is what the build without the bad edges gives), and a caller is expected to discard the
 * build, as PropGraph does (IndexError).
 * ------------------------------------------------------------------------------------- */
size_t lgc_build_workspace_bytes(int64_t n_nodes, int64_t n_edges);

int lgc_build_csr(const int64_t *edge_index, const float *edge_weight,
                  int64_t n_nodes, int64_t n_edges,
                  int32_t by_source, int32_t normalize,
                  const float *dis_in,
                  int32_t *rowptr, lgc_entry *entries,
                  float *edge_val, float *deg_out, float *dis_out,
                  void *workspace, size_t workspace_bytes,
                  int32_t *status, void *stream);

/* The user|item split of an edge list in the layout of src/utils_v2.py:146-165 (ids below n_users are users): out2[0] =
 * max over edges of min(source, target), out2[1] = min over edges of max(source, target) (int64 [2], device).  The graph is
 * user|item with split = out2[0] + 1 iff out2[0] < out2[1].  One pass over the COO. */
int lgc_bipartite_split(const int64_t *edge_index, int64_t n_edges, int64_t *out2, void *stream);

/* The work list of lgc_spmm's long rows, built on the device: every row of [row_begin, row_end) with more than `short_max`
 * entries is cut into ceil(deg / chunk_len) near-equal chunks, listed in row order; a row with several chunks gets
 * consecutive partial-sum slots and an lgc_multi_row.  lgc_row_plan_count leaves per-row prefix sums in `workspace`
 * (>= lgc_row_plan_workspace_bytes(n_rows)) and writes totals[3] = {chunks, multi-chunk rows, slots} (int32, device);
 * the caller sizes `chunks` and `multi` from them and calls lgc_row_plan_fill with the same arguments and workspace. */
size_t lgc_row_plan_workspace_bytes(int64_t n_rows);
int lgc_row_plan_count(const int32_t *rowptr, int32_t row_begin, int32_t row_end, int32_t short_max, int32_t chunk_len,
                       void *workspace, size_t workspace_bytes, int32_t *totals, void *stream);
int lgc_row_plan_fill(const int32_t *rowptr, int32_t row_begin, int32_t row_end, int32_t short_max, int32_t chunk_len,
                      const void *workspace, lgc_chunk *chunks, lgc_multi_row *multi, void *stream);

/* ---------------------------------------------------------------------------------------
 * Tiled rows: rows with at most 32 entries, listed in a caller-chosen processing order.
 *
 * Same arithmetic as lgc_spmm's short rows -- the gather -> scale -> scatter-add of one PyG LGConv layer,
 * called from src/lightgcn.py:96 (and the epilogue of src/lightgcn.py:93,97) -- for the rows of `order`,
 * entries in edge order, products rounded before the add.  lgc_build_tiles copies those rows into the tile
 * layout: 1 KiB pieces (2 KiB for width 32) that one coalesced access per wavefront fetches, holding
 * 128 / width (width 32: 8) whole rows each, padding entries col = -1 -- the hop reads no row pointer.
 *   order    int32 [n_slots]: row ids, -1 = empty slot; n_slots a multiple of the rows per tile R
 *            (16 for width 8, 8 for width 16 and 32); every listed row must have at most `width` entries.
 *            Slot g * (R/4) + bt of a tile is processed by lane group g in batch bt.
 *   meta     int32 [n_tiles]: byte bt = the largest entry count among the four rows of batch bt (upper bounds
 *            are allowed), or NULL.  With meta, a 61..64- or 68..128-wide table and tables below 4 GiB the kernel takes
 *            the path without divergent control flow (DPP broadcasts, buffer addressing); otherwise a generic one.
 *   width    8, 16 or 32 entries per row
 *   y[row] = a * sum_k val_k * x[col_k] + b * r[row]   (r may be NULL)
 */
int lgc_build_tiles(const int32_t *rowptr, const lgc_entry *entries, const int32_t *order, int64_t n_slots,
                    int32_t width, lgc_entry *slab, void *stream);

/* The processing order itself, on the device (what the host code otherwise derives with two dozen index operations):
 * lgc_tile_classes sorts the rows of [row_begin, row_end) by (width class, key, row id) -- class 0 / 1 / 2 = at most
 * min(8 | 16 | 32, max_len) entries (a row goes to the narrowest class that holds it; 0 entries -> class 0), class 3 = every
 * longer row; key = (popularity of the row's least-gathered column, that column) when `cold`, else nothing (row order) --
 * into sorted_rows (int32 [n_rows]) and counts the classes (class_count uint64 [4], device).  lgc_tile_pack turns one
 * class's slice of sorted_rows into `order` (int32 [n_tiles * R], -1 padded; inside a tile the longest rows first, rank
 * rho in slot (rho % 4) * R / 4 + rho / 4) and `meta` (int32 [n_tiles], byte bt = longest row of batch bt), n_tiles =
 * ceil(n_rows / R), R = 16 (width 8) or 8.  table_rows bounds the column ids; workspace >= the _workspace_bytes answer.
 * One-time planning calls, not hop launches: with `cold`, lgc_tile_classes reads the entry range of the rows back and
 * synchronises `stream` once (like lgc_sweep_plan_upload, lgc_sweep_dplan_create and lgc_sweep_dplan_fill, which say so). */
size_t lgc_tile_classes_workspace_bytes(int64_t n_rows, int64_t table_rows);
int lgc_tile_classes(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end, int32_t max_len,
                     int32_t cold, int64_t table_rows, void *workspace, size_t workspace_bytes, int32_t *sorted_rows,
                     uint64_t *class_count, void *stream);
int lgc_tile_pack(const int32_t *rowptr, const int32_t *sorted_rows, int64_t n_rows, int32_t width, int32_t *order, int32_t *meta,
                  void *stream);

int lgc_spmm_tiles(const int32_t *order, const int32_t *meta, const lgc_entry *slab, int32_t n_tiles, int32_t width,
                   int32_t tiles_per_wave, int64_t table_rows, const float *x, int64_t x_stride,
                   float *y, int64_t y_stride, const float *r, int64_t r_stride, float a, float b, int32_t dim,
                   void *stream);

/* ---------------------------------------------------------------------------------------
 * One propagation hop:  y[row] = a * sum_k entries[k].val * x[entries[k].col] + b * r[row]
 * for row in [row_begin, row_end) and for the rows named by `chunks`.
 *
 * Replaces one LGConv.forward (src/lightgcn.py:96) and, through a/b/r, the layer sum of
 * src/lightgcn.py:93,97 folded into the epilogue (r may be NULL: then y = a * sum).
 *
 *   rows with at most `short_max` entries in [row_begin,row_end) are done by one lane group
 *   each, accumulating in entry order; longer rows there are skipped and must appear in
 *   `chunks` (one wavefront per chunk).  Chunks with slot >= 0 write raw sums to
 *   partials[slot * dim ...]; `multi` rows then add their slots in order and apply the
 *   epilogue, which makes the result independent of scheduling.
 *
 *   table_rows  number of rows of the x / y / r tables (every row and column index is below it)
 *   x, y, r     fp32, row strides in floats (>= dim); any dword-aligned rows are accepted, 16-byte
 *               aligned rows (dim % 4 == 0) are the fast case;  y must not alias x
 *   partials    fp32 [n_slots, dim] or NULL when no chunk has slot >= 0
 * ------------------------------------------------------------------------------------- */
int lgc_spmm(const int32_t *rowptr, const lgc_entry *entries,
             int32_t row_begin, int32_t row_end, int32_t short_max,
             const lgc_chunk *chunks, int32_t n_chunks,
             const lgc_multi_row *multi, int32_t n_multi, float *partials,
             int64_t table_rows,
             const float *x, int64_t x_stride,
             float *y, int64_t y_stride,
             const float *r, int64_t r_stride,
             float a, float b, int32_t dim, void *stream);

/* The hop of lgc_spmm for a short LIST of rows:  y[row] = a * sum_k val_k * x[col_k] + b * r[row]  for row in row_ids
 * (int64 [n_ids], device; ids outside [row_begin, row_end) are skipped, repeats are harmless), every other row of y left
 * untouched.  One wavefront per listed row; rows of up to 32 entries are summed in entry order (the bits of lgc_spmm /
 * lgc_spmm_tiles), longer ones strided over the lane groups.  What it is for: `LightGCN.forward` in a training step scores
 * 2B label pairs (src/lightgcn.py:123-125, src/train_lightgcn.py:138), so of the last user step's output only the rows
 * of the batch's users are ever read -- a few thousand gathers instead of the whole 1.6 M-row step. */
int lgc_spmm_rows(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end, const int64_t *row_ids,
                  int64_t n_ids, int64_t table_rows, const float *x, int64_t x_stride, float *y, int64_t y_stride, const float *r,
                  int64_t r_stride, float a, float b, int32_t dim, void *stream);

/* The same for a list that names LONG rows (ABI 12).  What it is for: the scores of a training step read the propagated
 * table at the batch's 2B item rows too (src/lightgcn.py:123-125: `out[edge_label_index[1]]`), and nothing else of the last
 * item step's [n_items, D] block is ever read -- but an item row holds 186 entries on average and a hub beyond 10^5, which
 * one wavefront per row cannot balance.  The listed rows are cut into chunks ON THE DEVICE (no host round trip, fixed launch
 * shapes: the step can be recorded as a HIP graph): a one-workgroup planning launch (entries of the listed rows -> chunk
 * length: 256 entries, or longer when `partial_rows` would not hold that many chunks -> first chunk number of every list
 * position), a fixed grid of wavefronts striding over the chunk numbers (rows of up to 32 entries finish in entry order
 * with the bits of lgc_spmm_tiles; longer single-chunk rows finish directly; the others leave partial rows), and one
 * wavefront per cut position adding its partial rows by lane group: deterministic, no float atomics.
 *   order of the sums   G = 64 / lanes per row lane groups (lanes per row = ceil(dim / 4) from 4 columns up, else dim).
 *                 A span of more than 32 entries -- a whole row of one chunk, or one chunk -- hands entry k to lane group
 *                 (k - begin) % G; every group adds its entries in order from +0, the group sums are added as
 *                 ((g0 + g1) + g2) + ...  The partial rows of a cut position are added the same way: its j-th chunk by lane
 *                 group j % G, each group in order from +0, then the groups in order.  That is plain chunk order only
 *                 where G = 1, from 129 columns up.  lgc_spmm_rows sums every longer row as ONE span, so the two agree bit
 *                 for bit on rows of one chunk and differ in association on cut rows.
 *   y_rows        rows of y (compact: >= n_ids; else > every listed id of the operator half, i.e. >= row_end)
 *   compact       0: y[row_ids[m]] is written (as lgc_spmm_rows); 1: y[m] is written -- a [n_ids, dim] table in list order
 *                 (positions whose id lies outside [row_begin, row_end) are left untouched), e.g. the block a rank of a
 *                 partition all-reduces instead of the whole item block
 *   work          int32 [n_ids + 2] device scratch
 *   partials      fp32 [partial_rows, dim] device scratch, partial_rows > n_ids (LGC_E_RANGE otherwise); n_ids + 16384
 *                 keeps 256-entry chunks up to 4 M listed entries
 * r (optional epilogue rows) is indexed by row id in both modes.  Three launches on `stream`. */
int lgc_spmm_rows_split(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end,
                        const int64_t *row_ids, int64_t n_ids, int64_t table_rows, const float *x, int64_t x_stride, float *y,
                        int64_t y_stride, int64_t y_rows, const float *r, int64_t r_stride, float a, float b, int32_t dim,
                        int32_t compact, int32_t *work, float *partials, int64_t partial_rows, void *stream);

/* ---------------------------------------------------------------------------------------
 * Band sweep: long rows over a gathered table far larger than the caches (the item step of a user|item graph).
 *
 * Same hop as lgc_spmm's chunked rows (one LGConv layer, src/lightgcn.py:96, epilogue of :93,97), organised so that a
 * row of the gathered table crosses the memory fabric about once per pass instead of once per use: the columns
 * [col_lo, col_hi) are cut into n_bands ranges (one per XCD), every (row, band) pair gets an accumulator in LDS, and
 * all wavefronts of a band walk its columns in ascending order together.  Sums are taken per piece in column order
 * and per row in band order: deterministic, different association from lgc_spmm (inside the 1e-5 gate).
 *
 * The plan is built on the HOST from host copies of the CSR (the only entry points that take host pointers):
 *   lgc_sweep_plan_create  rows [row_begin, row_end) of the CSR; returns NULL and sets *code on error
 *   lgc_sweep_plan_dims    sizes of the arrays below
 *   lgc_sweep_plan_export  copies them into caller-provided HOST buffers:
 *       slabs uint32 [n_slabs * 64 * groups], wave_slab_ptr int32 [n_waves + 1], wave_npieces int32 [n_waves],
 *       piece_slot int32 [n_waves * row_cap], multi lgc_multi_row [n_rows]
 *   lgc_sweep_plan_free
 * The caller uploads the arrays and passes device pointers to lgc_spmm_sweep, with a scratch `partials` of
 * n_slots * dim floats.  The rows of `multi` may be split over two lists: `multi` (one lane group per row, for rows
 * with few slots) and `multi_wide` (one wavefront per row, for rows cut into many pieces); every row in exactly one.  lgc_sweep_ok says whether a table qualifies (< 2^24 - 1 rows, < 4 GiB) and with which plan: 4 (entries per step) for 61..64 columns and for 97..128 columns (the same plan run twice, columns [0, 64) and [64, dim)), 2 for 68..96 columns, 0 = no sweep.
 */
typedef struct lgc_sweep_cfg {
    int32_t n_bands;               /* 8: one band per XCD (blockIdx % 8)                               */
    int32_t waves_per_band_round;  /* 256: 32 CUs x 8 wavefronts                                       */
    int32_t row_cap;               /* 78: accumulators per wavefront (8 x 79 rows x 256 B = 158 KiB; 51 for 68..96 columns) */
    int32_t piece_cap;             /* 64: longest run of one row's entries inside one wavefront's list; raised in
                                      steps of 16 (up to 4x) while that saves a whole round                */
    int32_t lookahead;             /* 64: how far the step builder looks for an entry of another piece  */
    int32_t groups;                /* entries per step = table rows a wavefront gathers per instruction: 4 (or 0) for tables
                                      of 61..64 columns (a 16-lane group per row, 1 KiB slabs), 2 for 68..96 columns (two
                                      DPP rows per row, 512-byte slabs)                                                   */
    int32_t round_order;           /* which pieces of a band share a round.  0: every round gets the same mix (pieces dealt
                                      heaviest-first over all wavefronts of the band); 1: the heaviest pieces fill round 0,
                                      the next round 1, ... (dealt heaviest-first inside the round).  A column's table row
                                      is fetched once per round that holds a piece using it, so grouping the long pieces
                                      leaves the later rounds touching few columns: 576 -> 551 us per hop on the
                                      1.6 M x 54 k graph; 2: as 1, and the odd rounds walk their band in descending column
                                      order (a round starts where the previous one ended, on rows still in the Infinity
                                      Cache: another 2 us per hop).  Entries of a piece are then accumulated in
                                      descending column order in odd rounds (still one fixed order per plan)              */
    int32_t light_len;             /* light rows: a row with at most this many entries IN TOTAL gets one piece per PAIR of
                                      adjacent bands (2k, 2k+1) instead of one per band.  The piece lives in a wavefront of its
                                      home band 2k + (row & 1) (row counted from row_begin), or in the band that has the
                                      entries if the other run is empty; that wavefront gathers the neighbour band's columns
                                      too, each sorted into the band's walk at its position relative to its own band
                                      (bound[home] + (col - bound[own]) * width(home) / width(own)).  Fewer pieces: fewer
                                      partial rows and possibly a round less.  0 = off (the plan of before, array for array);
                                      > 0 needs an even n_bands (LGC_E_INVAL otherwise); -1 = the planner chooses: the smallest
                                      length, up to twice the median row length, with which the plan takes one round less and
                                      its most-loaded band fills at most 97 % of the remaining rounds, else 0 (also for odd
                                      n_bands).  lgc_sweep_dims.light_len reports the length in force                        */
} lgc_sweep_cfg;

typedef struct lgc_sweep_dims {
    int32_t n_bands, rounds, row_cap, piece_cap, n_rows, groups;
    int64_t n_waves, n_slabs, n_slots, n_entries, n_steps, n_padding;
    int32_t light_len, reserved;   /* the light-row length the plan was built with (cfg.light_len, resolved if it was -1) */
} lgc_sweep_dims;

typedef struct lgc_sweep_plan lgc_sweep_plan;

lgc_sweep_plan *lgc_sweep_plan_create(const int32_t *rowptr_host, const lgc_entry *entries_host, int32_t row_begin,
                                      int32_t row_end, int32_t col_lo, int32_t col_hi, const lgc_sweep_cfg *cfg,
                                      int *code);
int lgc_sweep_plan_dims(const lgc_sweep_plan *plan, lgc_sweep_dims *dims);
int lgc_sweep_plan_export(const lgc_sweep_plan *plan, uint32_t *slabs, int32_t *wave_slab_ptr, int32_t *wave_npieces,
                          int32_t *piece_slot, lgc_multi_row *multi);
/* The four big arrays straight into caller-provided DEVICE buffers of the sizes lgc_sweep_plan_dims reports (slabs,
 * wave_slab_ptr, wave_npieces, piece_slot; `multi` stays with lgc_sweep_plan_export: the host splits it by slot count);
 * synchronises `stream` before returning, so the plan may be freed right away.  Spares a host copy of ~90 MB. */
int lgc_sweep_plan_export_multi(const lgc_sweep_plan *plan, lgc_multi_row *multi);      /* HOST buffer, [n_rows] */
int lgc_sweep_plan_upload(const lgc_sweep_plan *plan, uint32_t *slabs, int32_t *wave_slab_ptr, int32_t *wave_npieces,
                          int32_t *piece_slot, void *stream);
void lgc_sweep_plan_free(lgc_sweep_plan *plan);

/* The same plan -- bit for bit -- with the bulk of the work on the device (rows [row_begin, row_end) of a CSR that is
 * ALREADY on the device; first_entry / n_entries = rowptr[row_begin] and the entry count of the range, which the caller
 * knows): column histogram, every row sorted by column (one radix sort), the run length of every (row, band); on the host
 * only the piece list and the deal over the wavefronts (from the run lengths, ~2 MB); back on the device every
 * wavefront's merged column-sorted list (a second radix sort) and the conflict-free step builder, one wavefront per list
 * (its look-ahead window is the wavefront's 64 lanes).  The 81 MB of entries are never copied to the host and the 87 MB of
 * slabs never from it.  Needs cfg->piece_cap <= 64 and cfg->lookahead <= 64 (LGC_E_RANGE otherwise: use the host planner).
 * cfg->light_len as in the host planner (the list order of a light row's entries in its neighbour band is the sort key's
 * 24-bit column field; the slabs carry the entries' own columns).
 *   lgc_sweep_dplan_create   everything up to the sizes (returns NULL and sets *code on error); `workspace` (device,
 *                            >= lgc_sweep_dplan_workspace_bytes) must stay untouched until _fill has returned
 *   lgc_sweep_dplan_dims     as lgc_sweep_plan_dims
 *   lgc_sweep_dplan_fill     writes the four arrays into caller-provided DEVICE buffers of those sizes; synchronises
 *   lgc_sweep_dplan_export_multi   `multi` into a HOST buffer [n_rows]; multi[].row are the CSR's own row ids
 *   lgc_sweep_dplan_free */
typedef struct lgc_sweep_dplan lgc_sweep_dplan;
size_t lgc_sweep_dplan_workspace_bytes(int64_t n_entries, int64_t n_rows, int64_t n_cols, const lgc_sweep_cfg *cfg);
lgc_sweep_dplan *lgc_sweep_dplan_create(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end,
                                        int64_t first_entry, int64_t n_entries, int32_t col_lo, int32_t col_hi,
                                        const lgc_sweep_cfg *cfg, void *workspace, size_t workspace_bytes, void *stream,
                                        int *code);
int lgc_sweep_dplan_dims(const lgc_sweep_dplan *plan, lgc_sweep_dims *dims);
int lgc_sweep_dplan_fill(const lgc_sweep_dplan *plan, uint32_t *slabs, int32_t *wave_slab_ptr, int32_t *wave_npieces,
                         int32_t *piece_slot, void *stream);
int lgc_sweep_dplan_export_multi(const lgc_sweep_dplan *plan, lgc_multi_row *multi);
void lgc_sweep_dplan_free(lgc_sweep_dplan *plan);

int lgc_sweep_ok(int32_t dim, int64_t table_rows, int64_t x_stride);

int lgc_spmm_sweep(const uint32_t *slabs, const int32_t *wave_slab_ptr, const int32_t *wave_npieces,
                   const int32_t *piece_slot, int64_t n_waves, int32_t row_cap, int32_t groups, const lgc_multi_row *multi,
                   int32_t n_rows, const lgc_multi_row *multi_wide, int32_t n_wide, float *partials, int64_t table_rows, const float *x, int64_t x_stride, float *y,
                   int64_t y_stride, const float *r, int64_t r_stride, float a, float b, int32_t dim, void *stream);
/* ---------------------------------------------------------------------------------------
 * One operator half as a single argument, and the per-hop exchange hook.
 *
 * lgc_operator gathers everything one `y[rows] = a * A[rows, :] x + b * r[rows]` needs -- the chunk plan of
 * lgc_spmm, the tile classes of lgc_spmm_tiles and, when the half qualifies, the band-sweep arrays -- so that a
 * host applies it with ONE call (lgc_apply picks the path exactly as the separate entry points would:
 * sweep if `sweep` is set and lgc_sweep_ok(dim, table_rows, x_stride); else chunks + tiles; tiles need dim >= 4,
 * narrower tables take lgc_spmm's row part over [row_begin, row_end)).
 *
 * lgc_apply_route answers, on the host and without launching anything, which of these routes lgc_apply takes for a
 * table geometry (lgc_apply decides by calling it): one LGC_ROUTE_* code, with LGC_ROUTE_WT_STORE OR-ed in while
 * y's byte offsets fit 32 bits (table_rows * y_stride * 4 < 2^32: output rows leave through write-through buffer
 * stores; plain stores beyond), or LGC_E_*.  r_stride = 0: no r.  Only `op` and the HOST struct `op->sweep` are read.
 * The DPP tile bodies and the sweep need 24-bit row ids, 32-bit byte offsets and the padding id 0xFFFFFF's wrapped
 * offset beyond the table, so the route depends on table_rows and the strides, not on the width alone.
 * The switches LGCN_NO_FAST_TILES (no DPP tile bodies) and LGCN_NO_FUSED_APPLY (chunks and tile classes as separate
 * launches) and LGCN_SWEEP_LAUNCH_WAVES (the sweep in launches of that many wavefronts) are read from the environment
 * ONCE per process, at the first hop or route query; later changes to the environment are not seen.
 */
#define LGC_ROUTE_ROWS           1   /* lgc_spmm's rows: no tile classes, or dim < 4                                 */
#define LGC_ROUTE_SWEEP          2   /* band sweep, 4 entries per step (61..64 columns) + fixed-order combine        */
#define LGC_ROUTE_SWEEP_WIDE     3   /* band sweep, 2 entries per step (68..96 columns) + combine                    */
#define LGC_ROUTE_SWEEP_TWO_PASS 4   /* the 4-entry sweep over columns [0, 64) and [64, dim) (97..128) + combine     */
#define LGC_ROUTE_FUSED_DPP      5   /* one launch of chunks + tile classes, DPP tile bodies (61..64, 68..128)       */
#define LGC_ROUTE_FUSED_GENERIC  6   /* one launch of chunks + tile classes, generic tile body                      */
#define LGC_ROUTE_SPLIT_DPP      7   /* LGCN_NO_FUSED_APPLY: lgc_spmm's chunks, then lgc_spmm_tiles per class, DPP  */
#define LGC_ROUTE_SPLIT_GENERIC  8   /* LGCN_NO_FUSED_APPLY, generic tile body                                       */
#define LGC_ROUTE_WT_STORE   0x100   /* bit: output rows through sc1 buffer stores with 32-bit offsets               */

/*
 * lgc_hop_exchange is one LGConv layer (src/lightgcn.py:96) of a user|item graph PARTITIONED over several devices
 * (SURVEY.md 8e): item step (partial sums of all item rows from this rank's own users) -> `exchange(block, rows,
 * row_stride, dim, stream, user)` -> user step (this rank's users from the replicated, now reduced, item rows).
 * The callback must leave the SUM over ranks in `block` (y rows [exchange_row_begin, +exchange_rows), row stride
 * y_stride floats) in stream order -- e.g. ncclAllReduce(block, block, rows * row_stride, ncclFloat, ncclSum, comm,
 * stream) when y_stride == dim -- and return 0; it is the only place where the library needs the host's
 * communicator, which it never sees.  A non-zero return aborts the hop and is handed back.
 * `item_epilogue`: the exchanged block is a SUM over ranks, so the b * r term of the item rows may enter it once only:
 * pass 1 on exactly one rank (rank 0) and 0 on the others -- with the same r and b everywhere; the user step applies
 * the epilogue of this rank's own user rows on every rank.
 */
typedef struct lgc_tile_class {
    const int32_t   *order;      /* device, [n_tiles * R]            */
    const int32_t   *meta;       /* device, [n_tiles] or NULL        */
    const lgc_entry *slab;       /* device, lgc_build_tiles layout   */
    int32_t n_tiles, width;
} lgc_tile_class;

typedef struct lgc_sweep_arrays {
    const uint32_t *slabs;
    const int32_t  *wave_slab_ptr, *wave_npieces, *piece_slot;
    const lgc_multi_row *multi, *multi_wide;
    float   *partials;           /* [n_slots, dim] scratch            */
    int64_t  n_waves;
    int32_t  row_cap, n_rows, n_wide;
    int32_t  groups;             /* 4 (or 0): plan for 61..64 columns; 2: plan for 68..96 columns */
} lgc_sweep_arrays;

typedef struct lgc_operator {
    const int32_t   *rowptr;
    const lgc_entry *entries;
    const lgc_chunk *chunks;
    const lgc_multi_row *multi;
    float   *partials;           /* scratch of the chunk plan, [n_slots, dim] or NULL */
    const lgc_sweep_arrays *sweep;   /* HOST pointer or NULL */
    lgc_tile_class tiles[3];
    int32_t row_begin, row_end, short_max, n_chunks, n_multi, n_tile_classes, tiles_per_wave, reserved;
} lgc_operator;

int lgc_apply_route(const lgc_operator *op, int64_t table_rows, int64_t x_stride, int64_t y_stride, int64_t r_stride,
                    int32_t dim);
int lgc_apply(const lgc_operator *op, int64_t table_rows, const float *x, int64_t x_stride, float *y, int64_t y_stride,
              const float *r, int64_t r_stride, float a, float b, int32_t dim, void *stream);

/*
 * lgc_apply with a SECOND epilogue row, on the three sweep routes only:
 *     y[row] = (b2 * r2[row] + b * r[row]) + a * (A x)[row]
 * every product rounded before its add, in this association -- the bits of lgc_apply(x, t) followed by
 * lgc_lincomb(y, {(b2, r2), (b, r), (a, t)}), without the table t and the second launch: the item step before the last
 * layer writes the layer sum the last user step gathers (bipartite_sum).  The sweep runs as in lgc_apply; the combine is
 * k_sweep_combine with the two-row epilogue.  r and r2 are both required (LGC_E_INVAL for either missing or a stride below dim,
 * LGC_E_ALIGN for one that is not dword aligned); r may alias y as in lgc_apply (a lane reads the elements it then writes),
 * r2 may too.  The route is asked of lgc_apply_route first: its errors come back unchanged, and an operator that would not take
 * LGC_ROUTE_SWEEP / _SWEEP_WIDE / _SWEEP_TWO_PASS at this geometry is refused with LGC_E_DIM before anything is launched.
 */
int lgc_apply2(const lgc_operator *op, int64_t table_rows, const float *x, int64_t x_stride, float *y, int64_t y_stride,
               const float *r, int64_t r_stride, const float *r2, int64_t r2_stride, float a, float b, float b2, int32_t dim,
               void *stream);

typedef int (*lgc_exchange_fn)(float *block, int64_t rows, int64_t row_stride, int32_t dim, void *stream, void *user);

int lgc_hop_exchange(const lgc_operator *item_op, const lgc_operator *user_op, int64_t table_rows, const float *x,
                     int64_t x_stride, float *y, int64_t y_stride, const float *r, int64_t r_stride, float a, float b,
                     int32_t dim, int32_t exchange_row_begin, int32_t exchange_rows, int32_t item_epilogue,
                     lgc_exchange_fn exchange, void *user, void *stream);

/* Fixed-order sum of runs -- how the sparse gradient of a scoring step (src/lightgcn.py:123-125 scores 2B pairs; what
 * autograd's index_select backward does with float atomics at src/train_lightgcn.py:146) is accumulated deterministically:
 * `key_sorted` int64 [n] is sorted; position t is a head when key[t] != key[t - 1]; for every head with 0 <= dest[t] < y_rows
 *   y[dest[t]] = (accumulate ? y[dest[t]] : 0) + scale * (vals[t] + vals[t + 1] + ... over the run, in that order)
 * vals fp32 [n, dim] dense.  One lane group owns a destination row: no atomics, the same bits on every run. */
int lgc_segment_sum(const int64_t *key_sorted, const int64_t *dest, const float *vals, const int32_t *vals_index, int64_t n,
                    float scale, float *y, int64_t y_stride, int64_t y_rows, int32_t dim, int32_t accumulate, void *stream);
/* vals_index (int32 [n] or NULL): the value row of sorted position t is vals[vals_index[t]] -- the permutation a sort
 * returned, so that the value table is never copied into sorted order. */

/* ---------------------------------------------------------------------------------------
 * The glue of one training step (src/train_lightgcn.py:137-147) around the propagation, as a handful of launches instead
 * of the ~150 small torch kernels the same arithmetic costs on the host side: on a rank of an 8-way partition the step was
 * bound by the host's launch rate (3.0 ms wall for 1.5 ms of kernels).
 *
 * lgc_pair_dot_rows  lgc_pair_dot that also keeps what autograd's backward of src/lightgcn.py:123-125 needs: the two
 *                    gathered rows of every pair (rows0, rows1: fp32 [n_pairs, dim] dense, or NULL) and a validity byte
 *                    (ok: uint8 [n_pairs] or NULL; 0 for an out-of-range pair, whose rows are zeros and whose score is NaN).
 * lgc_bpr_loss       `recommendation_loss(pos, neg, 0) * size` (src/lightgcn.py:262-286, src/train_lightgcn.py:141) for
 *                    scores [2 * n_triples] = [pos | neg] and its gradient: loss[0] = -sum_{mask} log sigmoid(pos - neg) /
 *                    size, grad [2 * n_triples].  mask (uint8 [n_triples] or NULL = all): the triples this caller owns --
 *                    a rank of a partition scores the triples of its own users; `size` is the GLOBAL batch size.
 * lgc_pair_seed_vals the sparse gradient of the scores with respect to the propagated table, as rows of a value table:
 *                    vals[m] = g_m * rows1[m], vals[n_pairs + m] = g_m * rows0[m], g_m = mask[m] ? grad_scores[m] *
 *                    (*grad_scale) : 0 (grad_scale: DEVICE scalar or NULL; mask uint8 [n_pairs] or NULL).
 * lgc_seed_prepare   sorts the m <= LGC_SEED_MAX node ids `rows` (int64; ids outside [0, n_nodes) count as "no row" and
 *                    come out as -1, first; two launches: every id ranked by counting, then one thread per sorted position)
 *                    and derives, per sorted position t: rows_sorted[t]; perm[t] (int32, the input
 *                    position: a stable sort); dest_item[t] = the row if t heads a run of an item row (row >= split) else
 *                    -1; dest_slot[t] = t, dest_user[t] = the row if t heads a run of a user row (row < split) else -1 --
 *                    the three destination lists of lgc_segment_sum for the item block of the seed table, the compact
 *                    table of seed users and the user rows of the result.  With col_flag / col_slot (both or neither):
 *                    col_flag[row] = 1, col_slot[row] = t for every user head -- lgc_seed_pull's column map.
 * lgc_seed_flags     col_flag[row] = value for the user rows of a sorted list (value 0 takes the flags back).
 * ------------------------------------------------------------------------------------- */
#define LGC_SEED_MAX 8192
int lgc_pair_dot_rows(const float *emb, int64_t stride, int32_t dim, int64_t n_nodes, const int64_t *idx0, const int64_t *idx1,
                      int64_t n_pairs, float *scores, float *rows0, float *rows1, uint8_t *ok, int32_t *status, void *stream);
int lgc_bpr_loss(const float *scores, const uint8_t *mask, int64_t n_triples, int64_t size, float *loss, float *grad,
                 void *stream);
/* The regulariser of src/utils_v2.py:193-211 (called at src/train_lightgcn.py:142) in one launch (ABI 12):
 *   value[0] = scale * (|w[ids0]|_F^2 + |w[ids1]|_F^2 + |w[ids2]|_F^2)      scale = decay / (2 * batch_size)
 * each norm as (sqrt(sum of squares))^2 like `init_embed[batch].norm().pow(2)`; ids int64 device lists of m0 / m1 / m2
 * entries (a list may be empty), negative ids wrap like torch's indexing.  rows_out (int64 [m0 + m1 + m2] or NULL): the ids
 * as row numbers in list order -- the rows the regulariser's gradient decay / size * w[row] goes to (lgc_segment_sum); an id
 * outside [-n_rows, n_rows) contributes nothing, comes out as -1 ("no row") and sets LGC_ST_INDEX_OOB in `status` (upstream's
 * gather raises IndexError).  One workgroup, fixed reduction order: the same bits on every run. */
int lgc_reg_rows(const float *w, int64_t stride, int32_t dim, int64_t n_rows, const int64_t *ids0, int64_t m0, const int64_t *ids1,
                 int64_t m1, const int64_t *ids2, int64_t m2, float scale, float *value, int64_t *rows_out, int32_t *status,
                 void *stream);

int lgc_pair_seed_vals(const float *grad_scores, const uint8_t *mask, const float *grad_scale, const float *rows0,
                       const float *rows1, int64_t n_pairs, int32_t dim, float *vals, void *stream);
int lgc_seed_prepare(const int64_t *rows, int64_t m, int64_t split, int64_t n_nodes, int64_t *rows_sorted, int32_t *perm,
                     int64_t *dest_item, int64_t *dest_slot, int64_t *dest_user, uint8_t *col_flag, int32_t *col_slot,
                     uint64_t *scratch /* [m], device */, void *stream);
int lgc_seed_flags(const int64_t *rows_sorted, int64_t m, int64_t split, uint8_t *col_flag, int32_t value, void *stream);

/* Seeded pull (first hop of the backward pass, loss.backward() at src/train_lightgcn.py:146): the incoming gradient has
 * non-zero rows only at a few thousand seed columns, given as a compact table.  The hop of lgc_spmm over rows
 * [row_begin, row_end) + chunks, in which an entry counts only if col_flag[col] != 0 and then gathers row col_slot[col] of
 * `seed_vals` (fp32 [n_seed, seed_stride]):   y[row] = sum_{k : col_flag[col_k]} val_k * seed_vals[col_slot[col_k]].
 * Same fixed summation order as lgc_spmm (entry order per lane group, chunk slots in order): deterministic, where a push
 * along the seeds' rows needs float atomics.  col_flag uint8 [table_rows], col_slot int32 [table_rows] (read only where
 * the flag is set). */
int lgc_seed_pull(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end, int32_t short_max,
                  const lgc_chunk *chunks, int32_t n_chunks, const lgc_multi_row *multi, int32_t n_multi, float *partials,
                  const uint8_t *col_flag, const int32_t *col_slot, const uint8_t *row_mark, const float *seed_vals,
                  int64_t seed_stride, int64_t table_rows, float *y, int64_t y_stride, int32_t dim, void *stream);

/* Which rows the seeded pull has to read at all: a batch of B users touches ~6 B of the 54 k item rows, and scanning the
 * other rows' 10 M entries for flags that are not there was 227 of the pull's 240 us.  lgc_seed_mark walks the rows listed
 * in `seed_rows` (int64 [n_seed], sorted; ids outside [row_begin, row_end) are skipped, repeats are harmless) of the
 * operator half that HOLDS the seeds -- the user rows, for a seed of users -- and stores `value` (0..255) in mark[col] for
 * each of their columns col < mark_len.  lgc_seed_pull given `row_mark` (uint8 [table_rows], NULL = read every row)
 * writes rows whose mark is 0 as zeros without reading their entries; value 0 takes the marks back after the pull. */
int lgc_seed_mark(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end, const int64_t *seed_rows,
                  int64_t n_seed, uint8_t *mark, int64_t mark_len, int32_t value, void *stream);

/* y[i, :dim] = sum_t coef[t] * src[t][i, :dim]  for i < n_rows, terms added in index order, each product
 * rounded before its add -- the order of the reference's running layer sum `out = out + x * alpha`
 * (src/lightgcn.py:93,97).  `src`, `src_stride`, `coef` are HOST arrays of n_terms (1..LGC_MAX_TERMS) entries;
 * src[t] are device pointers.  y may alias one of the sources (element-wise). */
#define LGC_MAX_TERMS 8
int lgc_lincomb(float *y, int64_t y_stride, const float *const *src, const int64_t *src_stride,
                const float *coef, int32_t n_terms, int64_t n_rows, int32_t dim, void *stream);

/* ---------------------------------------------------------------------------------------
 * Dense Adam step over a contiguous fp32 table in ONE pass (w, g, m, v read once; w, m, v written once): what
 * `optimizer.step()` of `torch.optim.Adam(model.parameters(), lr)` does at src/train_lightgcn.py:58,147 (amsgrad off, no
 * weight decay):  m <- m + (g - m)(1 - beta1);  v <- beta2 v + (1 - beta2) g^2;
 *                 w <- w - step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with step_size = lr / (1 - beta1^t) and bias_correction2_sqrt = sqrt(1 - beta2^t) computed by the host (t = step
 * count), and (1 - beta1), (1 - beta2) handed over as the host rounds them from double, like torch's own scalars
 * (1.0f - 0.999f is 4.7e-5 away from 0.001f).  n elements each; the four pointers dword-aligned and at the SAME offset
 * inside a 16-byte line (LGC_E_ALIGN otherwise) -- 16-byte aligned tables, or the same row range of same-shaped tables:
 * a rank of a partitioned run updates only the rows it owns (its users + the item block), two calls per step.
 * ------------------------------------------------------------------------------------- */
int lgc_adam_step(float *w, const float *g, float *m, float *v, int64_t n, float one_minus_beta1, float beta2,
                  float one_minus_beta2, float eps, float step_size, float bias_correction2_sqrt, void *stream);
/* The same with the six scalars read from DEVICE memory: hyper = {1 - beta1, beta2, 1 - beta2, eps, step_size,
 * bias_correction2_sqrt} (fp32 [6]).  For launches captured in a HIP graph and replayed every step: step_size and
 * bias_correction2_sqrt change with the step count, so the host refreshes those 24 bytes before each replay. */
int lgc_adam_step_hp(float *w, const float *g, float *m, float *v, int64_t n, const float *hyper, void *stream);

/* ---------------------------------------------------------------------------------------
 * Pair scoring: scores[m] = <emb[idx0[m]], emb[idx1[m]]>.
 * Replaces src/lightgcn.py:123-125.  idx are the rows of edge_label_index
 * (src/utils_v2.py:184-190), int64.  Out-of-range pairs score NaN and set LGC_ST_INDEX_OOB.
 * ------------------------------------------------------------------------------------- */
int lgc_pair_dot(const float *emb, int64_t stride, int32_t dim, int64_t n_nodes,
                 const int64_t *idx0, const int64_t *idx1, int64_t n_pairs,
                 float *scores, int32_t *status, void *stream);

/* Serving tail of LightGCN.recommendK (src/lightgcn.py:175-177; called per request from
 * torchserve/lightgcn_handler.py:91): masked = scores * (1 - seen), then per row the k largest by
 * (value descending, index ascending), entirely on the device -- upstream copies the [rows, n_cols] score matrix
 * to the host first.  The full order: every NaN (either sign bit) first, then +inf, the finite values with -0 = +0,
 * then -inf; equal elements by ascending index.  k <= 256 (LGC_E_RANGE beyond).  The mask comes in one of two forms (or neither: NULL, NULL):
 *   dense   seen fp32 [n_rows, n_cols], any values -- what upstream's handler builds per request
 *           (index_select on the sparse purchase matrix + to_dense, lightgcn_handler.py:88);
 *   lists   list_ptr int64 [n_users + 1], list_items int64 (a CSR of the purchase matrix, seen = 1 for listed
 *           columns), list_rows int64 [n_rows] = the user of each score row (NULL: row r is user r): the kernel
 *           builds a bit per column in LDS, the dense mask never exists (n_cols <= 983,040).
 *   scores fp32 [n_rows, n_cols] (row stride in floats), out_index int64 [n_rows, k], out_value fp32 [n_rows, k] or NULL. */
int lgc_mask_topk(const float *scores, int64_t score_stride, const float *seen, int64_t seen_stride,
                  const int64_t *list_ptr, const int64_t *list_items, const int64_t *list_rows, int64_t n_rows,
                  int32_t n_cols, int32_t k, int64_t *out_index, float *out_value, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fold-in: the embedding of a node that is NOT a row of the trained table -- a visitor the model has never seen, or a
 * known user whose list changed after training -- from the items it interacted with.  Upstream has no such path: its
 * handler gathers a trained row per requested id (torchserve/lightgcn_handler.py:73-96) out of the table that
 * `get_embedding` propagates (src/lightgcn.py:91-99), and an id outside the table raises.  What this computes is exactly
 * the row src/lightgcn.py:91-99 gives a node appended to the trained graph with ONE-WAY edges i_k -> node (weights w_k) and
 * layer-0 row z; one-way edges leave every existing degree and row untouched:
 *     out[r] = a0 * init[init_rows[r]] + sum_k c_k * fold[i_k],   c_k = item_dis[i_k] * w_k * d,   d = (sum_k w_k)^-1/2
 * with fold = sum_{l=0..K-1} alpha_{l+1} * x_l[items], one [n_items, dim] table per model and graph (the caller computes it
 * once: the layer sum with the coefficients shifted by one).
 *   list_ptr    int64 [n_rows + 1], list_items int64: the lists as a CSR of item indices in [0, n_items) WITHOUT the
 *               n_users offset -- lgc_mask_topk's list form with list_rows = NULL, so the same two arrays mask the scores.
 *               list_ptr is read on trust (as lgc_mask_topk reads its lists)
 *   list_weight fp32 per entry, or NULL = all ones
 *   item_dis    fp32 [n_items]: the item slice of the graph's dis (lgc_build_csr's dis_out); required with normalize = 1,
 *               ignored with normalize = 0 (then c_k = w_k)
 *   fold        fp32 [n_items, dim], rows fold_stride floats apart; n_items >= 1
 *   init_rows   int64 [n_rows] or NULL: an id in [0, n_init_rows) adds a0 * init[id] (init fp32, rows init_stride apart);
 *               -1 = no row; any other id sets LGC_ST_INDEX_OOB and adds nothing
 *   out         fp32 [n_rows, dim], rows out_stride apart; EVERY row is written: an empty list, or one whose weights sum
 *               to 0 (d = 0, as lgc_build_csr's dis), gives a0 * init or zeros
 * Arithmetic (the build's and the hop's own, so the identity holds to rounding): the degree is the fp32 sum of the list's
 * weights taken sequentially in list order; d = 1 / sqrt(deg), both correctly rounded, inf -> 0; c_k = (item_dis * w) * d left
 * to right, each product rounded; every product is rounded before its add; the a0 * init term is added last.  An item
 * outside [0, n_items) is skipped altogether -- it is left out of the degree too -- and sets LGC_ST_INDEX_OOB; the index is
 * range-checked before any address is formed from it.  Negative weights behave as in lgc_build_csr.  Lists of up to 32
 * entries are summed in list order (the short-row contract of lgc_spmm / lgc_spmm_tiles); longer ones in a fixed order
 * that depends only on dim and the pointers' alignment.  No float atomics: the same bits on every run.
 * One wavefront per row; 16-byte loads where dim % 4 == 0 and all rows are 16-byte aligned, dword loads otherwise.
 * Errors before any launch: LGC_E_DIM (as lgc_dim_ok); LGC_E_INVAL (a null required pointer, a negative size, n_items < 1,
 * a stride below dim, normalize outside {0, 1}, normalize = 1 without item_dis, init_rows without init); LGC_E_RANGE
 * (n_rows or n_items >= 2^31).  n_rows == 0 validates, launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
int lgc_fold_in(const int64_t *list_ptr, const int64_t *list_items, const float *list_weight, int64_t n_rows,
                const float *item_dis, const float *fold, int64_t fold_stride, int64_t n_items,
                const int64_t *init_rows, const float *init, int64_t init_stride, int64_t n_init_rows, float a0,
                int32_t normalize, int32_t dim, float *out, int64_t out_stride, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Epoch evaluation (TrainLightGCN.test, src/train_lightgcn.py:155-162: recommendK over all validation users,
 * then MARK_MAPK): scores, ranking and metrics in bounded device memory.  A caller walks its users in panels:
 * lgc_score_rows -> lgc_mask_topk (list form, list_rows = the panel's users) per panel, then lgc_topk_hits and
 * lgc_metric_sums once.
 *
 * lgc_score_rows: out[r, i] = sum_d users[row_ids[r], d] * items[i, d], a dense fp32 panel.
 *   users    fp32 [n_user_rows, dim], rows user_stride floats apart (>= dim; columns past dim are never read)
 *   row_ids  int64 [n_rows], any order, repeats allowed; NULL = row r is user row r.  An id outside
 *            [0, n_user_rows) sets LGC_ST_INDEX_OOB in `status` and zero-fills its row; nothing is read out of range
 *   items    fp32 [n_items, dim], rows item_stride floats apart
 *   dim      as lgc_dim_ok (LGC_E_DIM otherwise)
 *   out      fp32 [n_rows, n_items], rows out_stride floats apart (>= n_items)
 * The bits of out[r, i] depend only on the two source rows and dim: one chain of fused multiply-adds over d in
 * ascending order.  They do not depend on r, i, n_rows, n_items, the strides or how a request is cut into panels. */
int lgc_score_rows(const float *users, int64_t user_stride, int64_t n_user_rows, const int64_t *row_ids,
                   int64_t n_rows, const float *items, int64_t item_stride, int32_t n_items, int32_t dim,
                   float *out, int64_t out_stride, int32_t *status, void *stream);

/* hits[r] = number of entries of topk[r, 0..k) that occur in the positive list of the row's user, and
 * recall[r] = hits[r] / (pos_ptr[u + 1] - pos_ptr[u]) -- MARK_MAPK's per-user columns (src/lightgcn.py:184-190).
 *   topk       int64 [n_rows, k], rows topk_stride apart, entries of a row distinct (lgc_mask_topk's output);
 *              k <= 256 (LGC_E_RANGE beyond)
 *   pos_ptr / pos_items   int64 [n_users + 1] / int64: the positive lists as a CSR.  A positive listed twice hits
 *              once (upstream intersects sets) but counts twice in the denominator (upstream's len of the list);
 *              an empty list gives recall NaN (upstream divides by zero)
 *   list_rows  int64 [n_rows] = the user of each row (NULL: row r is user r), as in lgc_mask_topk; a user outside
 *              [0, n_users) sets LGC_ST_INDEX_OOB in `status`, hits 0 and recall 0
 *   hits int32 [n_rows], recall double [n_rows] */
int lgc_topk_hits(const int64_t *topk, int64_t topk_stride, int32_t k, const int64_t *pos_ptr,
                  const int64_t *pos_items, const int64_t *list_rows, int64_t n_rows, int64_t n_users,
                  int32_t *hits, double *recall, int32_t *status, void *stream);

/* *hits_sum = sum of hits[0..n_rows) (int64), *recall_sum = sum of recall[0..n_rows) (double), by one workgroup in a
 * fixed order: the same bits on every run.  Either output (with its input) may be NULL, not both.  n_rows == 0
 * writes nothing. */
int lgc_metric_sums(const int32_t *hits, const double *recall, int64_t n_rows, int64_t *hits_sum,
                    double *recall_sum, void *stream);

/* Ranking metrics per row at several cutoffs from ONE ranking: the rows of lgc_mask_topk are sorted by (value descending,
 * index ascending), so the first c entries of a top-k row are the top-c row.  Stands in for MARK_MAPK's per-user columns
 * (src/lightgcn.py:184-190: overlap_item, recall, precision) and adds what its name promises and it does not compute.
 *   topk, topk_stride, k, pos_ptr, pos_items, list_rows, n_rows, n_users, status   as lgc_topk_hits (entries of a row
 *              distinct; a user outside [0, n_users) sets LGC_ST_INDEX_OOB and every output of its row is 0)
 *   pos_distinct  int64 [n_users]: the number of DISTINCT items of each user's list (n below); NULL = the lists hold no
 *              duplicates and the list length is used.  len = pos_ptr[u + 1] - pos_ptr[u] counts duplicates
 *   cutoffs    int32 [n_cut] on the HOST, 1 <= n_cut <= LGC_RM_MAX_CUTOFFS, each >= 1, strictly ascending, the last <= k
 *              (LGC_E_INVAL otherwise; k or a cutoff above 256: LGC_E_RANGE)
 *   hit_bits   uint64 [n_rows, 4] or NULL: bit j of the row (bit j % 64 of word j / 64) is set when topk[r, j] occurs in
 *              the user's list; bits at and past k are zero.  rel_j below is bit j
 *   hits       int32 [n_rows, n_cut]: hits@c = the number of set bits below c
 *   metrics    double [n_rows, n_cut, LGC_RM_COUNT], per cutoff c:
 *     LGC_RM_PRECISION  hits@c / c
 *     LGC_RM_RECALL     hits@c / len                 (at c == k the bits of lgc_topk_hits' recall)
 *     LGC_RM_NDCG       DCG@c / IDCG@c,  DCG@c = sum_{j<c} rel_j d_j,  IDCG@c = sum_{j<min(c,n)} d_j,  d_j = 1 / log2(j + 2)
 *     LGC_RM_AP         (sum_{j<c} rel_j hits@(j+1) / (j+1)) / min(c, n)
 *     LGC_RM_RR         1 / (j0 + 1) for the lowest set bit j0 < c, else 0
 *     LGC_RM_HIT        1.0 if hits@c > 0, else 0.0
 * All arithmetic is double; d_j is a table the host computes once.  Every sum over j is a running sum in ascending j and a
 * cutoff is a snapshot of it: the value at cutoff c does not depend on k, n_cut or the other cutoffs, bit for bit.  An
 * empty list gives NaN in recall, NDCG and AP (0 / 0, as upstream's division).  No float atomics: the same bits on
 * every run.  Nothing is read through a topk entry; entries are only compared. */
#define LGC_RM_PRECISION 0
#define LGC_RM_RECALL    1
#define LGC_RM_NDCG      2
#define LGC_RM_AP        3
#define LGC_RM_RR        4
#define LGC_RM_HIT       5
#define LGC_RM_COUNT     6
#define LGC_RM_MAX_CUTOFFS 8
int lgc_rank_metrics(const int64_t *topk, int64_t topk_stride, int32_t k, const int64_t *pos_ptr,
                     const int64_t *pos_items, const int64_t *pos_distinct, const int64_t *list_rows, int64_t n_rows,
                     int64_t n_users, const int32_t *cutoffs, int32_t n_cut, uint64_t *hit_bits, int32_t *hits,
                     double *metrics, int32_t *status, void *stream);

/* out[c] = sum over r of in[r, c] for a double [n_rows, n_cols] matrix, rows in_stride doubles apart: the means of
 * MARK_MAPK (src/lightgcn.py:184-190, the two .mean() calls) for every metric column at once.  Per column the additions
 * run in lgc_metric_sums' order (thread t adds rows t, t + 1024, ..., then a binary tree), so the sum of a recall column
 * has the bits of lgc_metric_sums' recall_sum.  n_cols <= LGC_COLUMN_SUMS_MAX (LGC_E_RANGE beyond).  No atomics.
 * n_rows == 0 writes nothing. */
#define LGC_COLUMN_SUMS_MAX 64
int lgc_column_sums(const double *in, int64_t in_stride, int64_t n_rows, int32_t n_cols, double *out, void *stream);

/* Catalogue coverage per cutoff: how many distinct items the first c entries of all rows touch (upstream has no such
 * number; a caller of MARK_MAPK, src/lightgcn.py:184-190, would count the union of its top_rlvnt_itm lists on the host).
 *   topk, topk_stride, k, n_rows   as lgc_rank_metrics; cutoffs, n_cut as there (the same error codes)
 *   n_items    entries are item indices in [0, n_items); n_items >= 1 (LGC_E_INVAL otherwise), below 2^31 (LGC_E_RANGE)
 *   bitmap     uint32 [n_cut, ceil(n_items / 32)], zeroed by the caller before the FIRST call: row ci gets, by integer
 *              atomic OR, a bit for every item among the first cutoffs[ci] entries of every row
 *   counts     int64 [n_cut]: overwritten with the number of set bits of the whole bitmap row -- a second call with
 *              further rows (the next request) and the same bitmap accumulates
 *   status     an entry outside [0, n_items) sets LGC_ST_INDEX_OOB and marks nothing (it is range-checked before any
 *              address is formed from it) */
int lgc_topk_coverage(const int64_t *topk, int64_t topk_stride, int32_t k, int64_t n_rows, const int32_t *cutoffs,
                      int32_t n_cut, int64_t n_items, uint32_t *bitmap, int64_t *counts, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Hop distances and shortest paths from users to their recommended items (InferenceLightGCN.compute_paths,
 * src/inference_lightgcn.py:85-119: per pair has_path + shortest_path_length + shortest_path of networkx on the host).
 * Here: a level-synchronous BFS from up to LGC_BFS_MAX_SOURCES sources at once over the forward CSR of lgc_build_csr
 * (row v lists the sources j of the edges j -> v: the pull direction of the search and the predecessor list of the
 * walk back).  Bit containers are uint64 words, one per node: bit b of seen[v] = "source b has reached v".  Entry
 * values are ignored: an edge of weight 0 or of negative weight is an edge.  All results are integers; they are the same
 * bits on every run (the only atomics are integer OR and integer counts).
 *
 * lgc_bfs_init      seen[v] = frontier[v] = 0 for v < n_nodes, then bit b set at sources[b] in both (int64 [n_sources];
 *                   two sources may name one node: both bits are set).  A source outside [0, n_nodes) sets
 *                   LGC_ST_INDEX_OOB in `status` and no bit.
 * lgc_bfs_level     for every row v of [row_begin, row_end):
 *                       fresh = (OR over the row's columns j of frontier_in[j]) & ~seen[v]
 *                       frontier_out[v] = fresh;  seen[v] |= fresh
 *                   by the row plan of lgc_spmm: rows of at most `short_max` entries by a lane group each, longer rows per
 *                   chunk of `chunks` (every longer row must be listed), one wavefront each; a row cut into several chunks
 *                   (slot >= 0) combines them with 64-bit atomic OR.  A row with (~seen[v] & active) == 0 -- `active` =
 *                   the mask of the batch's valid source bits -- is finished without reading its entries: frontier_out[v]
 *                   = 0, seen[v] unchanged.  Any other row gets all of `fresh`: it is masked by seen[v], not by `active`.
 *                   A bit of frontier_in outside `active` therefore travels like any other, with one exception the caller
 *                   must not rely on: a row cut into several chunks may drop such bits (a chunk that finds the row finished
 *                   by a sibling chunk of the same level is skipped as well); bits inside `active`, and the count of new
 *                   nodes, never depend on the cut or on timing.  paths.py keeps frontier_in inside `active`: a source
 *                   outside the graph sets no bit.  Rows outside [row_begin, row_end) are neither read nor written.  active
 *                   == 0 launches nothing.  frontier_out must not be frontier_in.  The launch ADDS to `counters` (uint64 [4],
 *                   zeroed by the caller): [0] += nodes newly reached, [2] |= their new bits, i.e. the sources whose
 *                   frontier is not empty after this level; [1] belongs to lgc_bfs_resolve, [3] is reserved.
 * lgc_bfs_resolve   for every pair (b, c) with dist[b, c] == LGC_BFS_UNSET (int32 [n_sources, n_targets], filled with it by
 *                   the caller): dist = level if bit b of frontier[targets[b, c]] is set (targets int64 [n_sources,
 *                   n_targets]).  A source or target outside [0, n_nodes): LGC_ST_INDEX_OOB, dist = -1.  counters[1] +=
 *                   pairs settled by this call, so the caller knows how many are still unset.
 * lgc_bfs_backtrack one shortest path per pair with 0 <= d = dist[b, c] < min(n_levels, path_len), from `levels` (uint64
 *                   [n_levels, n_nodes]: row l = the frontier_out of level l, row 0 = lgc_bfs_init's frontier):
 *                   paths[b, c, d] = the target, and for l = d - 1 ... 0 paths[b, c, l] = the first column, in the stored
 *                   entry order of the row of paths[b, c, l + 1], that has bit b set in levels[l].  Positions past d, and
 *                   the whole row of every other pair, are -1.  paths int64 [n_sources, n_targets, path_len].
 *
 * More than LGC_BFS_MAX_SOURCES sources, or n_nodes / n_targets that do not fit int32: LGC_E_RANGE.  No sources or no
 * targets: nothing is launched.
 * ------------------------------------------------------------------------------------- */
#define LGC_BFS_MAX_SOURCES 64
#define LGC_BFS_UNSET (-3)     /* dist of a pair no level has settled yet (-1 and -2 are results: see paths.py) */
int lgc_bfs_init(const int64_t *sources, int32_t n_sources, int64_t n_nodes, uint64_t *seen, uint64_t *frontier,
                 int32_t *status, void *stream);
int lgc_bfs_level(const int32_t *rowptr, const lgc_entry *entries, int32_t row_begin, int32_t row_end, int32_t short_max,
                  const lgc_chunk *chunks, int32_t n_chunks, uint64_t active, const uint64_t *frontier_in,
                  uint64_t *frontier_out, uint64_t *seen, uint64_t *counters, void *stream);
int lgc_bfs_resolve(const int64_t *sources, const int64_t *targets, int32_t n_sources, int64_t n_targets, int64_t n_nodes,
                    const uint64_t *frontier, int32_t level, int32_t *dist, uint64_t *counters, int32_t *status,
                    void *stream);
int lgc_bfs_backtrack(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, const uint64_t *levels,
                      int32_t n_levels, const int64_t *targets, const int32_t *dist, int32_t n_sources, int64_t n_targets,
                      int64_t *paths, int32_t path_len, void *stream);

/* ---------------------------------------------------------------------------------------
 * Mini-batch sampler: for each of the `n` given users one positive and one negative item.
 * Replaces the per-row Python of batch_loader (src/utils_v2.py:168-181; its caller
 * src/train_lightgcn.py:132): `p = random.choice(item_id_idx_list)`,
 * `n = rejection-sample random.randint(0, n_items-1) + n_users until not in ignor_neg_list`.
 * The users themselves (random.sample without replacement, :174) are drawn by the caller.
 *
 *   users       int64 [n]   user ids (rows of the two CSRs below)
 *   pos_ptr/pos_items   int32 [n_users+1] / int64 [..]  each user's positive item ids (already offset by
 *                       n_users, duplicates allowed: the choice is uniform over list entries, as upstream)
 *   ign_ptr/ign_items   int32 [n_users+1] / int64 [..]  each user's ignore set, SORTED ascending per user
 *   seed, step  the draw is a pure function of (seed, step, position in the batch): counter-based RNG
 *   pos_out, neg_out    int64 [n]
 *   status      LGC_ST_INDEX_OOB for a user id outside [0, n_users) or without positives;
 *               LGC_ST_SAMPLER_EXHAUSTED when 256 draws all hit the ignore set (then neg = last draw)
 * ------------------------------------------------------------------------------------- */
#define LGC_ST_SAMPLER_EXHAUSTED 2
int lgc_sample_triples(const int64_t *users, int64_t n,
                       const int32_t *pos_ptr, const int64_t *pos_items,
                       const int32_t *ign_ptr, const int64_t *ign_items,
                       int64_t n_users, int64_t n_items, uint64_t seed, uint64_t step,
                       int64_t *pos_out, int64_t *neg_out, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Middle-hop reduction of a user|item graph (an addition to ABI 14: exports only).
 *
 * Between two item steps of the layer loop (src/lightgcn.py:96 called K times) the user table is only a relay:
 * x_{l+1}[items] = R^T (R x_{l-1}[items]).  A user u with few entries costs a row store and as many gathers from the big
 * user table as from the small item table; taking the users L = {u : its row has <= max_deg entries AND <= max_deg item
 * rows name it} out of the CSR and keeping their two-step paths as  G_L = R_L^T R_L  (item x item, sparse) gives
 *     R^T R = R_H^T R_H + G_L
 * with H the kept users.  G_L depends on the graph and its values only: built once, beside the tile classes and the sweep
 * plan.  Both counts are taken because the edge list is never assumed structurally symmetric.
 *
 * Compact numbering: kept users keep their relative order as rows 0 .. n_kept-1, item i (node split + i) is row and
 * column n_kept + i; with offset = split - n_kept, row r of a table view that starts at row `offset` of a full table is
 * the compact node r, and the item rows sit where the full operators address them.
 *
 *   lgc_reduce_count      user_map (int32 [split]): new id of a kept user, -1 of an eliminated one; totals (int64 [4],
 *                         device) = {n_kept, entries of the kept user rows, entries of the whole reduced CSR, expanded
 *                         (item, item) pairs}.  Leaves prefix sums in `workspace` (>= lgc_reduce_workspace_bytes(n_nodes,
 *                         n_edges), 256-byte aligned), which the other calls read: keep it untouched until they returned.
 *                         The caller reads the totals back (the one sync) and sizes the outputs from them.
 *   lgc_reduce_fill       the reduced CSR: rowptr_out int32 [n_kept + n_items + 1], entries_out [n_out = totals[2]].  User
 *                         rows hold their entries with the columns renumbered, item rows only their entries on kept users;
 *                         values are bit-identical copies and the entry order inside a row is preserved.
 *   lgc_reduce_gram_count expands every entry (i, u) of an item row with u eliminated by u's row into keys (i, j) and fp64
 *                         products A[i, u] * A[u, j], sorts them (one stable 64-bit radix sort) and counts the distinct
 *                         keys: *total (int64, device) = nnz(G_L).  gram_workspace >= lgc_reduce_gram_workspace_bytes(n_pairs)
 *                         (0 = does not fit), n_pairs = totals[3]; n_pairs >= 2^31 - 1: LGC_E_RANGE -- run without elimination.
 *   lgc_reduce_gram_fill  G_L as a CSR over the same numbering: rowptr_out int32 [n_kept + n_items + 1] (user rows empty),
 *                         entries_out [n_out = *total], columns ascending within a row, diagonal included; each value the
 *                         fp64 sum of its products in expansion order (CSR order of the item entries, then of the user's
 *                         row), rounded once to fp32.  No float atomics: two builds of one input are bit-identical.
 * Argument errors come back before anything is enqueued: LGC_E_INVAL (null pointer, negative size, split outside (0, n_nodes),
 * n_out outside its range), LGC_E_RANGE, LGC_E_WORKSPACE, LGC_E_ALIGN.  rowptr / entries are read on trust like every
 * CSR the library built itself; an entry whose column is on the wrong side of the split is dropped.
 * ------------------------------------------------------------------------------------- */
size_t lgc_reduce_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int lgc_reduce_count(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, int64_t n_edges, int64_t split,
                     int32_t max_deg, void *workspace, size_t workspace_bytes, int32_t *user_map, int64_t *totals,
                     void *stream);
int lgc_reduce_fill(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, int64_t n_edges, int64_t split,
                    const void *workspace, const int32_t *user_map, int64_t n_kept, int64_t n_out, int32_t *rowptr_out,
                    lgc_entry *entries_out, void *stream);
size_t lgc_reduce_gram_workspace_bytes(int64_t n_pairs);
int lgc_reduce_gram_count(const int32_t *rowptr, const lgc_entry *entries, int64_t n_nodes, int64_t n_edges, int64_t split,
                          const void *workspace, int64_t n_pairs, void *gram_workspace, size_t gram_workspace_bytes,
                          int64_t *total, void *stream);
int lgc_reduce_gram_fill(const void *gram_workspace, int64_t n_pairs, int64_t n_kept, int64_t n_items, int64_t n_out,
                         int32_t *rowptr_out, lgc_entry *entries_out, void *stream);

/* The concatenated operator [R_H^T | G_L] (an addition to ABI 14: exports only): the item step of a reduced layer as ONE
 * operator, so that the entries of G_L run inside the kept users' band sweep instead of a launch of their own.  A sweep
 * entry's column is both its place in the band walk and the table row it gathers, so the rows of x_{l-2}[items] must sit
 * INSIDE the user part of table l-1, spread over the bands.  Physical numbering, from the outputs of lgc_reduce_fill /
 * lgc_reduce_gram_fill (compact numbering) alone:
 *   gap_rows = ceil(n_items / n_gaps);  n_phys = n_kept + n_gaps * gap_rows  (lgc_reduce_concat_rows);  rows 0 .. n_phys - 1
 *   are the kept users with n_gaps gaps of gap_rows rows between them, item i is row and column n_phys + i (so a view that
 *   starts at row split - n_phys of a full table has the item block where the full operators address it; the caller checks
 *   n_phys <= split).  Kept user h belongs to band floor(rowptr[h] * n_gaps / rowptr[n_kept]) (at most n_gaps - 1; band 0
 *   if the kept rows are empty) -- the share of the kept user rows' entries before it, which on a structurally symmetric
 *   graph is the sweep planner's own band rule applied to R_H^T -- and gap b follows the users of band b:
 *       user_pos[h]  = h + gap_rows * band(h)                                      int32 [n_kept]
 *       gap_start[b] = (kept users of bands 0 .. b) + gap_rows * b                 int32 [n_gaps]
 *   and item j owns row gap_start[j / gap_rows] + j % gap_rows (the last gap may keep up to n_gaps - 1 rows unused).
 *   rowptr_out  int32 [n_phys + n_items + 1], entries_out [n_out = n_entries + n_items + n_gram]:
 *     kept user rows   their entries in order, values bit-identical, columns moved behind the gaps;
 *     gap row of j     ONE entry {n_phys + j, 1.0f}: the user step that writes x_l[H] thereby also writes x_{l-1}[j] into its
 *                      gap (0 + 1.0f * v is v), and no launch is spent on filling the gaps; an unused gap row is empty;
 *     item row i       its entries on kept users (columns user_pos[h]) followed by its entries of G_L (columns = the gap
 *                      rows), values bit-identical.  Columns are NOT ascending within a row: the sweep planners sort.
 * n_gaps <= LGC_REDUCE_MAX_GAPS (LGC_E_RANGE).  Three launches of index arithmetic, no scan, no sort, no atomics.
 * lgc_reduce_concat_host is the same code on HOST arrays (every element is one call of the function the kernels call). */
#define LGC_REDUCE_MAX_GAPS 64
int64_t lgc_reduce_concat_rows(int64_t n_kept, int64_t n_items, int32_t n_gaps);     /* n_phys; -1 on a bad argument */
int lgc_reduce_concat(const int32_t *rowptr, const lgc_entry *entries, int64_t n_entries, const int32_t *gram_rowptr,
                      const lgc_entry *gram_entries, int64_t n_gram, int64_t n_kept, int64_t n_items, int32_t n_gaps,
                      int32_t *user_pos, int32_t *gap_start, int32_t *rowptr_out, lgc_entry *entries_out, int64_t n_out,
                      void *stream);
int lgc_reduce_concat_host(const int32_t *rowptr, const lgc_entry *entries, int64_t n_entries, const int32_t *gram_rowptr,
                           const lgc_entry *gram_entries, int64_t n_gram, int64_t n_kept, int64_t n_items, int32_t n_gaps,
                           int32_t *user_pos, int32_t *gap_start, int32_t *rowptr_out, lgc_entry *entries_out, int64_t n_out);

/* ---------------------------------------------------------------------------------------
 * Score attribution (an addition to ABI 14: exports only): which of a row's own items produced a recommendation.
 * Upstream's inference script stops at path lengths (src/inference_lightgcn.py:85-119).  Fold-in's line
 *     e_u = a0 * z_u + sum_k c_k * F[i_k]
 * dotted with a served item row E[t] splits every score additively over the row's list:
 *     score(u, t) = a0 <z_u, E[t]>  +  sum_k c_k <F[i_k], E[t]>  =  base[t] + sum_k contrib[k, t]
 * exactly (to rounding) for a session (c_k = lgc_fold_in's coefficient) and for a trained user (c_k = the value stored in
 * the user's row of the forward CSR, whose columns are the item nodes).  One launch, one workgroup per request row.
 *
 * The lists, in exactly ONE of two forms (LGC_E_INVAL for both or neither; the pointers of the other form NULL):
 *   session  list_ptr int64 [n_rows + 1], list_items int64, list_weight fp32 or NULL, item_dis, normalize: lgc_fold_in's
 *            arguments, and c_k with lgc_fold_in's arithmetic bit for bit (sequential fp32 degree in list order, correctly
 *            rounded 1 / sqrt with inf -> 0, (item_dis * w) * d left to right; normalize = 0: c_k = w_k).  An item outside
 *            [0, n_items) is left out of the degree, contributes nothing and sets LGC_ST_INDEX_OOB
 *   graph    rowptr int32, entries, row_ids int64 [n_rows], n_graph_rows, col_base: request row r is row row_ids[r] of the
 *            CSR, item index = col - col_base, c_k = val_k unchanged.  A row id outside [0, n_graph_rows) sets the status
 *            bit and every output of its row is the "nothing" value; a column outside [col_base, col_base + n_items) is
 *            skipped and flagged
 * Tables: fold (lgc_fold_in's F) and items (the served item rows E), fp32 [n_items, dim], row strides >= dim; init_rows /
 * init / init_stride / n_init_rows / a0 as in lgc_fold_in (-1 = no row, any other bad id is flagged and adds nothing);
 * targets int64 [n_rows, n_targets], rows target_stride apart: item indices, typically a row of lgc_mask_topk's output;
 * -1 = "no target" silently, any other value outside [0, n_items) sets the status bit, both give "nothing" in that column.
 * 1 <= n_targets <= LGC_ATTR_MAX_TARGETS, 0 <= top_m <= LGC_ATTR_MAX_TOP (LGC_E_RANGE beyond); dim as lgc_dim_ok.  Every
 * index is range-checked before an address is formed from it; lists and the CSR are read on trust.
 *
 * Outputs, each may be NULL but not all (top_m = 0 counts as no top output):
 *   contrib    fp32, ragged, with contrib_ptr int64 [n_rows + 1] = the first entry slot of each row (session form: list_ptr
 *              itself will do; graph form: the prefix sum of the row lengths): entry j of row r, target t goes to
 *              contrib[(contrib_ptr[r] + j) * n_targets + t]; at most contrib_ptr[r + 1] - contrib_ptr[r] entries of a
 *              row are written; a skipped entry writes +0
 *   base       fp32 [n_rows, n_targets] = a0 * dot(z, E[t]), +0 without an init row
 *   total      fp32 [n_rows, n_targets] = the contributions that count added SEQUENTIALLY IN LIST ORDER from +0, base last
 *   top_pos int32, top_item int64, top_value fp32, all [n_rows, n_targets, top_m]: the m contributions that rank first in
 *              lgc_mask_topk's total order on the value (NaN first, +inf, finite descending with -0 = +0, -inf), equal
 *              keys by ascending list position; top_pos counts skipped entries, which take no part; a repeated item
 *              stays two entries; unused places hold -1 / -1 / +0
 * "Nothing" value of a column or row: base = total = +0, top -1 / -1 / +0, contrib +0.
 * Arithmetic: dot(a, b) is lgc_score_rows' chain -- fused multiply-adds over d ascending from +0, zeros past dim -- so
 * dot(F[i], E[t]) has exactly the bits lgc_score_rows writes for that pair of rows; contrib = c_k * dot, one rounded
 * product.  No float atomics: the same bits on every run.
 * Errors before any launch: LGC_E_DIM; LGC_E_INVAL (a null required pointer, a negative size, n_items < 1, a stride below dim
 * or target_stride below n_targets, both or neither list form, normalize outside {0, 1} or 1 without item_dis, init_rows
 * without init, contrib without contrib_ptr, top_m > 0 without all three top pointers, no output at all); LGC_E_RANGE
 * (n_targets, top_m, n_rows or n_items >= 2^31); LGC_E_ALIGN (a table that is not dword aligned).  n_rows == 0 validates,
 * launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_ATTR_MAX_TARGETS 64
#define LGC_ATTR_MAX_TOP 8
typedef struct lgc_attr_args {          /* HOST struct of device pointers and sizes */
    const int64_t   *list_ptr, *list_items;                 /* session form */
    const float     *list_weight, *item_dis;
    const int32_t   *rowptr;                                /* graph form */
    const lgc_entry *entries;
    const int64_t   *row_ids;
    int64_t          n_graph_rows, col_base;
    int64_t          n_rows;
    const float     *fold, *items;
    int64_t          fold_stride, item_stride, n_items;
    const int64_t   *init_rows;
    const float     *init;
    int64_t          init_stride, n_init_rows;
    const int64_t   *targets;
    int64_t          target_stride;
    const int64_t   *contrib_ptr;
    float           *contrib, *base, *total;
    int32_t         *top_pos;
    int64_t         *top_item;
    float           *top_value;
    int32_t         *status;
    float            a0;
    int32_t          normalize, n_targets, top_m, dim;
} lgc_attr_args;

int lgc_attribute(const lgc_attr_args *args, void *stream);

/* ---------------------------------------------------------------------------------------
 * Similar items (an addition to ABI 14: exports only): "which items are like this one?" -- the k nearest rows of the item
 * table by dot product or cosine, for a product page's row of similar products, for deduplication and for diversity passes.
 * Upstream answers questions about users only (src/lightgcn.py:165-177).  Scoring runs on the fp32 matrix cores
 * (v_mfma_f32_16x16x4_f32) and the selection in the same launch: no score is written to memory.
 *
 * lgc_row_rnorm: out[r] = 1 / sqrt(sum_d table[r, d]^2), the scale that makes the dot product a cosine.
 *   table  fp32 [n_rows, dim], rows `stride` floats apart (>= dim); out fp32 [n_rows]
 *   ss is ONE chain ss = fma(x_d, x_d, ss) over d ascending from +0; the square root and the division are each correctly
 *   rounded; an infinite result becomes 0 (as lgc_build_csr's dis: a zero row is similar to nothing); NaN stays NaN.
 *   Errors: LGC_E_DIM; LGC_E_INVAL (null pointer, negative size, stride below dim); LGC_E_RANGE (n_rows >= 2^31);
 *   LGC_E_ALIGN (a pointer that is not dword aligned).  n_rows == 0 launches nothing.
 *
 * lgc_item_neighbors: per query row the k best candidates among the items.
 *   items      fp32 [n_items, dim], rows item_stride floats apart (>= dim; columns past dim are never read); n_items >= 1
 *   query_ids  int64 [n_queries] item indices, any order, repeats allowed; NULL = query r is item r.  An id outside
 *              [0, n_items) sets LGC_ST_INDEX_OOB in `status` and its whole row is -1 / -inf; it is range-checked before
 *              any address is formed from it
 *   scale      fp32 [n_items] or NULL: s = (dot * scale[query]) * scale[item], left to right, each product rounded; with
 *              scale = lgc_row_rnorm(items) that is the cosine, with NULL s = dot
 *   item_ok    uint8 [n_items] or NULL: an item with item_ok[i] == 0 is never returned (it may still be asked about)
 *   exclude_self  1: the query's own item is not a candidate; 0: it is
 *   k          1 .. LGC_NEIGHBORS_MAX_K
 *   slices     0 .. 64: the catalogue is cut into that many ranges of item tiles, one workgroup per (tile of 64 query rows,
 *              range), and a second small kernel merges the ranges' k best; 0 = the library chooses (the smallest count
 *              that gives about 512 workgroups: 1 for a whole catalogue, many for a request of a few ids); a count above
 *              the number of item tiles (128 items each) is clamped to it.  The result does not depend on it
 *   out_index  int64 [n_queries, k]; out_value fp32 [n_queries, k] or NULL.  With fewer than k candidates the tail of the
 *              row is -1 / -inf
 *   workspace  device memory of at least lgc_item_neighbors_workspace_bytes(n_queries, n_items, k, slices) bytes, 8-byte
 *              aligned; may be NULL where that is 0 (one range).  The size function returns 0 for sizes the call would
 *              refuse and grows monotonically in n_queries, n_items, k and in slices over 1 .. 64
 * Arithmetic: dot(q, i) is lgc_score_rows' chain -- fused multiply-adds over d ascending from +0, zeros past dim -- so it
 * has the bits lgc_score_rows writes for the same two rows, except that a sum of -0 may come out as +0 (the width is
 * padded with zeros to 16 columns); the order below does not tell them apart.
 * Order: lgc_mask_topk's total order -- every NaN (either sign bit) first, then +inf, the finite values descending with
 * -0 = +0, then -inf; equal elements by ascending index.  It is strict, so the result depends neither on the tile shape
 * nor on the slice count nor on the order in which candidates arrive.  A NaN comes back as the quiet NaN 0x7FFFFFFF and
 * -0 as +0.  No float atomics: the same bits on every run.
 * Errors before any launch: LGC_E_DIM (as lgc_dim_ok); LGC_E_INVAL (a null required pointer, a negative n_queries, a
 * stride below dim, exclude_self outside {0, 1}); LGC_E_RANGE (k outside 1 .. LGC_NEIGHBORS_MAX_K, slices outside
 * 0 .. 64, n_items < 1, n_items or n_queries >= 2^31); LGC_E_ALIGN (items, scale or out_value not dword aligned,
 * out_index or workspace not 8-byte aligned); LGC_E_WORKSPACE (a workspace that is too small or missing).
 * n_queries == 0 validates, launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_NEIGHBORS_MAX_K 64
int lgc_row_rnorm(const float *table, int64_t stride, int64_t n_rows, int32_t dim, float *out, void *stream);
size_t lgc_item_neighbors_workspace_bytes(int64_t n_queries, int64_t n_items, int32_t k, int32_t slices);
int lgc_item_neighbors(const float *items, int64_t item_stride, int64_t n_items, int32_t dim,
                       const int64_t *query_ids, int64_t n_queries, const float *scale, const uint8_t *item_ok,
                       int32_t exclude_self, int32_t k, int32_t slices, int64_t *out_index, float *out_value,
                       void *workspace, size_t workspace_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Diversified re-ranking (an addition to ABI 14: exports only): "give me k recommendations that are not k variants of one
 * product" -- greedy maximal marginal relevance (MMR, Carbonell & Goldstein 1998) over a candidate list, and the
 * intra-list diversity that judges the result.  Upstream ranks by score alone (src/lightgcn.py:175-177).  One launch, one
 * wavefront per row; the n_cand x n_cand similarity matrix of a list is never formed: k - 1 columns of it are.
 *
 * lgc_rerank_mmr: out of the n_cand candidates of every row, k in the order the greedy rule chooses them.
 *   items, item_stride, n_items, dim, scale   as lgc_item_neighbors (scale fp32 [n_items] or NULL)
 *   cand       int64 [n_rows, n_cand], rows cand_stride apart: item indices WITHOUT the n_users offset -- a row of
 *              lgc_mask_topk or lgc_item_neighbors.  -1 is an empty position and is skipped silently; any other id outside
 *              [0, n_items) is range-checked before an address is formed from it, skipped, and sets LGC_ST_INDEX_OOB.  A
 *              repeated id is two candidates: positions are what is chosen
 *   rel        fp32 [n_rows, n_cand], rows rel_stride apart: the relevance of each candidate, computed by the caller (the
 *              masked score: for recommendK's multiplicative mask a seen item is a candidate of relevance 0)
 *   n_cand     1 .. LGC_RERANK_MAX_CAND;  k  1 .. n_cand;  lambda in [0, 1]: 1 = relevance alone, 0 = diversity alone
 *   out_index  int64 [n_rows, k]: the items in the order chosen;  out_pos int32 [n_rows, k] or NULL: their positions in the
 *              candidate row;  out_value fp32 [n_rows, k] or NULL: the objective at the moment of choice, as compared (a NaN
 *              comes back as the quiet NaN 0x7FFFFFFF, -0 as +0).  A row with fewer than k valid positions ends in
 *              -1 / -1 / -inf
 * Arithmetic, bit for bit.  sim(i, j) for a remaining candidate of item i and the item j just chosen: dot(i, j) is
 * lgc_score_rows' chain -- fused multiply-adds over d ascending from +0, zeros past dim; the products commute, so
 * dot(i, j) = dot(j, i) -- and sim = (dot * scale[i]) * scale[j], left to right, each product rounded (lgc_item_neighbors'
 * rule with the remaining candidate in the query's place); with scale NULL sim = dot.  With oml = 1.0f - lambda in fp32:
 *   step 0     obj_p = lambda * rel_p for every valid position p;
 *   after the choice of position c, every valid position p not yet chosen: the first time pen_p = sim(p, c), afterwards
 *              pen_p = (s != s || s > pen_p) ? s : pen_p with s = sim(p, c) -- the running maximum; a NaN sticks;
 *   step t>=1  obj_p = (lambda * rel_p) - (oml * pen_p): two products and one subtraction, each rounded, nothing fused.
 * Every step chooses the best obj_p among the positions not yet chosen in lgc_mask_topk's total order -- every NaN first,
 * then +inf, the finite values descending with -0 = +0, then -inf -- equal objectives by ascending POSITION.  The order is
 * strict: the result depends on cand, rel, the item rows, scale and lambda alone, not on how positions are spread over
 * lanes, on the route or on the run.  No float atomics.  It follows that with lambda = 1 (and finite similarities: 0 * inf is
 * a NaN) the result is the first k positions of lgc_mask_topk's order over rel.
 * Routes: the candidate rows are staged once in LDS where n_cand * (dim rounded up to 4 * odd floats) * 4 bytes fit 36 KiB,
 * and read from memory at every step otherwise; lgc_rerank_route answers which (or LGC_E_DIM / LGC_E_RANGE), on the host.
 *
 * lgc_list_diversity: intra-list diversity of ranked lists at several cutoffs.
 *   lists      int64 [n_rows, k], rows list_stride apart; -1 and ids out of range as above; k <= LGC_RERANK_MAX_CAND
 *   cutoffs    int32 [n_cutoffs] on the HOST as lgc_rank_metrics takes them: 1 .. LGC_RM_MAX_CUTOFFS of them, each in 1 .. k,
 *              strictly ascending.  Positions at and past the last cutoff are not read
 *   out        double [n_rows, n_cutoffs], rows out_stride apart
 * For position b, t_b = the sum of (1.0 - (double) sim(a, b)) over the valid positions a < b, taken sequentially in
 * ascending a in float64 (sim as above with i = the earlier position a), 0 for an invalid b; S_c = the sum of t_b over
 * b < c, sequentially in ascending b; out[r, j] = S_c / (n_c (n_c - 1) / 2) with c = cutoffs[j] and n_c the valid positions
 * among the first c.  Fewer than two valid positions give NaN (as an empty positive list gives recall NaN).  The value at
 * a cutoff does not depend on k or on the other cutoffs.  Column means: lgc_column_sums.
 *
 * Errors of both, before any launch: LGC_E_DIM (as lgc_dim_ok); LGC_E_INVAL (a null required pointer, a negative n_rows,
 * a stride below its width, a lambda that is NaN, n_cutoffs < 1); LGC_E_RANGE (n_cand outside 1 .. LGC_RERANK_MAX_CAND, k
 * outside 1 .. n_cand resp. 1 .. LGC_RERANK_MAX_CAND, lambda outside [0, 1], n_items < 1, n_items or n_rows >= 2^31, more
 * than LGC_RM_MAX_CUTOFFS cutoffs, cutoffs not strictly ascending or outside 1 .. k); LGC_E_ALIGN (an fp32 or int32 pointer
 * that is not dword aligned, an int64 or double pointer that is not 8-byte aligned).  n_rows == 0 validates, launches
 * nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_RERANK_MAX_CAND 256          /* = lgc_mask_topk's k limit: a candidate list is one of its rows */
#define LGC_RERANK_ROUTE_LDS    1        /* the candidate rows are staged in LDS */
#define LGC_RERANK_ROUTE_GLOBAL 2        /* they are read from memory at every step */
int lgc_rerank_route(int32_t n_cand, int32_t dim);
int lgc_rerank_mmr(const float *items, int64_t item_stride, int64_t n_items, int32_t dim, const float *scale,
                   const int64_t *cand, int64_t cand_stride, const float *rel, int64_t rel_stride, int64_t n_rows,
                   int32_t n_cand, int32_t k, float lambda, int64_t *out_index, int32_t *out_pos, float *out_value,
                   int32_t *status, void *stream);
int lgc_list_diversity(const float *items, int64_t item_stride, int64_t n_items, int32_t dim, const float *scale,
                       const int64_t *lists, int64_t list_stride, int64_t n_rows, int32_t k, const int32_t *cutoffs,
                       int32_t n_cutoffs, double *out, int64_t out_stride, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Hard negatives (an addition to ABI 14: exports only): dynamic negative sampling for BPR.  A uniformly drawn negative
 * soon scores far below the positive and its gradient weight sigmoid(neg - pos) is almost nothing; here every sample
 * draws up to n_cand admissible candidates, scores them against the user's row of the given table and trains against the
 * highest-scored one.  One launch, one wavefront per sample; upstream's batch_loader (src/utils_v2.py:168-181) has no
 * counterpart.
 *
 *   users .. step   as lgc_sample_triples, and its stream exactly: sample i has
 *              key = mix64(mix64(seed) ^ mix64(step * STEP_MUL + i)), the positive is
 *              pos_items[pos_ptr[u] + bounded(mix64(key), count)], and attempt a = 1 .. 256 proposes the node
 *              n_users + bounded(mix64(key + ATTEMPT_MUL * a), n_items); an attempt is admissible when its node is not in
 *              the user's sorted ignore set (ign_items may be NULL where every set is empty)
 *   n_cand     1 .. LGC_HARDNEG_MAX_CAND.  The candidates of sample i are the first n_cand admissible attempts among
 *              attempts 1 .. 256, in attempt order: fewer where the 256 attempts hold fewer; a node drawn twice is two
 *              candidates and is scored twice
 *   user_table, user_stride   fp32 [n_users, dim], rows user_stride >= dim floats apart
 *   item_table, item_stride   fp32 [n_items, dim], rows item_stride >= dim apart: row c - n_users is node c's.  Columns at
 *              or past dim are never read: a row may end there
 *   pos_out, neg_out   int64 [n]: the positive, and the winner's node id
 *   neg_score  fp32 [n] or NULL: the winner's score;  neg_attempt int32 [n] or NULL: its attempt number, 1-based;
 *   n_admissible   int32 [n] or NULL: how many candidates were taken, 0 .. n_cand
 *   status     LGC_ST_INDEX_OOB, LGC_ST_SAMPLER_EXHAUSTED as lgc_sample_triples
 * Score, bit for bit.  The score of candidate c is dot(user_table[u], item_table[c - n_users]) with the bits lgc_score_rows
 * writes for those two rows: one chain of fp32 fused multiply-adds over d = 0 .. round_up(dim, 4) - 1, ascending from +0,
 * with zeros past dim.  neg_score is the chain's value (a -0 stays -0; any NaN stands for any NaN).
 * Winner.  The first element in lgc_mask_topk's total order over the candidates' scores -- every NaN first, then +inf, the
 * finite values descending with -0 = +0, then -inf -- equal scores going to the earlier attempt.  The order is strict: the
 * result depends on the arguments alone, not on how attempts are spread over lanes or rounds, nor on the run.  No float
 * atomics.  It follows that n_cand = 1 returns the pos_out and neg_out of lgc_sample_triples for the same arguments, and
 * that a table of zeros does so at any n_cand.
 * No admissible attempt among the 256: LGC_ST_SAMPLER_EXHAUSTED is set, neg_out[i] is the last draw as in
 * lgc_sample_triples, neg_attempt[i] = 256, n_admissible[i] = 0 and neg_score[i] is that draw's score.
 * A user outside [0, n_users) or without positives: LGC_ST_INDEX_OOB is set, pos_out[i] = neg_out[i] = n_users,
 * neg_score[i] = 0, neg_attempt[i] = 0, n_admissible[i] = 0; no table address is formed from the id.
 * Errors, before any launch: LGC_E_DIM (as lgc_dim_ok); LGC_E_INVAL (a null required pointer, a negative n, n_users < 0,
 * n_items < 1, a stride below dim); LGC_E_RANGE (n_cand outside 1 .. LGC_HARDNEG_MAX_CAND, or n or n_users + n_items
 * >= 2^31).  n == 0 validates, launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_HARDNEG_MAX_CAND 256         /* = the sampler's attempts: every attempt can be a candidate */
int lgc_sample_hard_triples(const int64_t *users, int64_t n,
                            const int32_t *pos_ptr, const int64_t *pos_items,
                            const int32_t *ign_ptr, const int64_t *ign_items,
                            int64_t n_users, int64_t n_items, uint64_t seed, uint64_t step, int32_t n_cand,
                            const float *user_table, int64_t user_stride,
                            const float *item_table, int64_t item_stride, int32_t dim,
                            int64_t *pos_out, int64_t *neg_out, float *neg_score, int32_t *neg_attempt,
                            int32_t *n_admissible, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Full-rank evaluation (an addition to ABI 14: exports only): "where in the whole catalogue did this held-out purchase
 * land?" -- per (user, item) pair the number of candidates that precede the item, which is what AUC, the mean percentile
 * rank and recall at any K are made of.  lgc_mask_topk answers only for the first 256 places.  A counting problem over
 * users x catalogue dot products: they run on the fp32 matrix cores (v_mfma_f32_16x16x4_f32) and end in integer counters in
 * registers; no score is written to memory.  Upstream has no counterpart (src/lightgcn.py:165-190 stops at the top k).
 *
 *   users, user_stride, n_user_rows   fp32 [n_user_rows, dim], rows user_stride >= dim floats apart
 *   items, item_stride, n_items       fp32 [n_items, dim], rows item_stride >= dim apart; n_items >= 1.  Columns at or past
 *              dim are never read: a row may end there
 *   pair_users, pair_items   int64 [n_pairs]: pair r = (u, p) asks for the place of item p in user u's ranking; any order,
 *              repeats allowed.  A user outside [0, n_user_rows) or an item outside [0, n_items) sets LGC_ST_INDEX_OOB in
 *              `status` and gives rank = n_equal = -1, n_cand = 0, value = 0; nothing is addressed through the id
 *   seen_ptr, seen_items   int64 [n_user_rows + 1] and int64: a CSR over all users, read on trust as lgc_mask_topk reads
 *              its lists; seen_ptr NULL = no lists, and seen_items is then ignored, its alignment too.  A user's items must be ascending (ingest.seen_csr, SeenLists.from_dense);
 *              an entry equal to its predecessor is skipped, one outside [0, n_items) is ignored.  An unsorted list gives
 *              unspecified counts but never an access out of range
 *   seen_mode  LGC_RANK_SEEN_ZERO: every item is a candidate and a seen one competes with m = score * 0 (one rounded
 *              multiply: +-0, and NaN for a seen +-inf) -- lgc_mask_topk's list form exactly, recommendK's ranking;
 *              LGC_RANK_SEEN_REMOVE: the seen items are no candidates (the usual LightGCN protocol).  A pair whose p is
 *              seen then gives rank = n_equal = -1 with n_cand and value (the raw score) still written and no status bit:
 *              a property of the data, not an error.  Without lists the two modes coincide
 *   slices     0 .. 64: the catalogue is cut into that many ranges of item tiles (128 items each), one workgroup per (tile
 *              of 64 pairs, range); 0 = the library chooses (about 512 workgroups), a count above the number of item tiles
 *              is clamped to it.  The result does not depend on it
 *   rank       int32 [n_pairs]: the number of candidates i != p with precedes(i, p)
 *   n_equal    int32 [n_pairs] or NULL: the number of candidates i != p whose key equals p's (degenerate ties show here)
 *   n_cand     int32 [n_pairs] or NULL: the number of candidates, p counted
 *   value      fp32 [n_pairs] or NULL: m(u, p)
 *   workspace  device memory of at least lgc_rank_positions_workspace_bytes(n_pairs, n_items, slices) bytes, dword aligned.
 *              The size function returns 0 for sizes the call would refuse and grows monotonically in n_pairs, n_items and
 *              in slices over 1 .. 64
 * Score: s(u, i) is lgc_score_rows' chain for the two rows -- fused multiply-adds over d ascending from +0, zeros past
 * dim -- with its bits, except that a sum of -0 may come out as +0 in a comparison (the order does not tell them apart);
 * `value` is the chain's own value.
 * Order: lgc_mask_topk's total order on the masked score m -- every NaN (either sign bit) first, then +inf, the finite
 * values descending with -0 = +0, then -inf; precedes(i, p): key(m_i) > key(m_p), or the keys are equal and i < p.  So in
 * mode ZERO rank[r] is the column of p in lgc_mask_topk's row for u wherever that row is long enough.
 * No float atomics; the slices add integers, whose sum does not depend on the order: the same bytes on every run.
 * Errors before any launch: LGC_E_DIM (as lgc_dim_ok); LGC_E_INVAL (a null required pointer, a negative n_pairs or
 * n_user_rows, a stride below dim, seen_mode outside {0, 1}, seen_ptr without seen_items); LGC_E_RANGE (slices outside
 * 0 .. 64, n_items < 1, n_items, n_pairs or n_user_rows >= 2^31 - 1); LGC_E_ALIGN (an fp32 or int32 pointer or the workspace
 * not dword aligned, an int64 pointer not 8-byte aligned); LGC_E_WORKSPACE (a workspace that is too small or missing).
 * n_pairs == 0 validates, launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_RANK_SEEN_ZERO   0
#define LGC_RANK_SEEN_REMOVE 1
size_t lgc_rank_positions_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t slices);
int lgc_rank_positions(const float *users, int64_t user_stride, int64_t n_user_rows,
                       const float *items, int64_t item_stride, int64_t n_items, int32_t dim,
                       const int64_t *pair_users, const int64_t *pair_items, int64_t n_pairs,
                       const int64_t *seen_ptr, const int64_t *seen_items, int32_t seen_mode,
                       int32_t slices,
                       int32_t *rank, int32_t *n_equal, int32_t *n_cand, float *value,
                       void *workspace, size_t workspace_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * In-batch softmax loss (an addition to ABI 14: exports only): a softmax (InfoNCE / sampled-softmax) objective over many
 * negatives per positive, for the rows a training batch has propagated anyway.  Every one of n_rows user rows is scored
 * against every one of n_cand listed items on the fp32 matrix cores (v_mfma_f32_16x16x4_f32); a user's own other positives
 * are no negatives (the sampler's ignore lists); out come the loss, the gradient of the logits and its two products with the
 * table rows, which are the gradient with respect to the propagated rows -- the seed of the sparse backward.  Five launches
 * in stream order.  Upstream trains BPR on one negative (src/train_lightgcn.py:137-147) and has no counterpart.
 *
 *   table, stride, table_rows, split, dim   fp32 [table_rows, dim], rows stride >= dim floats apart: the propagated table,
 *              user rows [0, split), item rows [split, table_rows).  Columns at or past dim are never read: a row may end there
 *   row_users  int64 [n_rows]: node ids in [0, split);  cand_items int64 [n_cand]: node ids in [split, table_rows), repeats
 *              allowed;  target int32 [n_rows]: the column of row i's positive
 *   ign_ptr, ign_items   int32 [split + 1] and int64: TripleSampler's ignore lists (node ids, ascending per user), read on
 *              trust as lgc_sample_triples reads them; both NULL = every list is empty
 *   cand_bias  fp32 [n_cand] or NULL: added to every logit of a column (-log q_j corrects for the sampling distribution)
 *   inv_tau    1 / temperature, finite and > 0;  size: the GLOBAL batch size, as in lgc_bpr_loss
 *   loss       fp32 [1];  row_loss fp32 [n_rows] or NULL;  n_adm int32 [n_rows] or NULL
 *   grad_logits, g_stride   fp32 [n_rows, n_cand], rows g_stride >= n_cand apart, or NULL (G then lives in the workspace)
 *   grad_users, grad_cands, grad_stride   fp32 [n_rows, dim] and [n_cand, dim], rows grad_stride >= dim apart.  Columns past
 *              dim of a gradient row are never written
 *   workspace  device memory of at least lgc_softmax_workspace_bytes(n_rows, n_cand) bytes, dword aligned (needed whether or
 *              not grad_logits is given).  The size function returns 0 for sizes the call would refuse and grows
 *              monotonically in both arguments
 * Logit.  s_ij = dot(table[row_users[i]], table[cand_items[j]]) is lgc_score_rows' chain for the two rows -- fp32 fused
 * multiply-adds over d ascending from +0, zeros past dim -- with its bits (a sum of -0 may come out as +0, which no result
 * here tells apart); z_ij = s_ij * inv_tau, one rounded multiply, then + cand_bias[j], one rounded add.
 * Admissible set.  With t = target[i], J_i holds t and every j != t whose cand_items[j] is a valid item id, differs from
 * cand_items[t] and is not in the ignore list of user row_users[i].
 * Results.  m_i = max_{J_i} z_ij;  S_i = sum_{J_i} exp(z_ij - m_i);  loss_i = (m_i - z_it) + log S_i, which is
 * log sum_{J_i} exp(z_ij - z_it);  *loss = (sum_i loss_i) / size, one fixed-order sum;  p_ij = exp(z_ij - m_i) / S_i;
 * G_ij = (p_ij - [j = t]) * (inv_tau / size) for j in J_i and exactly +0 for every other j;  grad_users[i] = sum_j G_ij
 * table[cand_items[j]];  grad_cands[j] = sum_i G_ij table[row_users[i]], both on the matrix cores with ONE accumulator per
 * element that takes the inner extent in ascending order;  n_adm[i] = |J_i| - 1.  A row with J_i = {t} has loss_i = +0 and a
 * zero row of G.  No float atomics: every output depends on the arguments alone, never on the run.
 * Bad ids.  A row whose user is outside [0, split), whose target is outside [0, n_cand) or whose cand_items[target] is no
 * item is invalid: loss_i = 0, n_adm = 0, zero rows of G and grad_users.  A candidate outside [split, table_rows) is
 * admissible for nobody and its grad_cands row is zeros.  Either sets LGC_ST_INDEX_OOB in `status`; every id is range-checked
 * before an address is formed from it.
 * Non-finite values.  z = -inf contributes 0 (a row whose admissible logits are ALL -inf gives NaN; a target at -inf beside
 * finite logits gives loss_i = +inf).  A NaN or +inf among a row's admissible logits gives NaN in row_loss[i], in every
 * admissible element of row i of G (the others stay +0), in grad_users[i] and in *loss, as a float64 evaluation of the
 * max-subtracted formula gives; n_adm is unaffected.  Such a row changes no other row's row_loss, G or grad_users; it does put
 * NaN into grad_cands[j] for every j it admits.  (A non-finite TABLE row of a candidate reaches every row's grad_users
 * through 0 * NaN, as in the float64 product.)
 * Every output element is written -- except with n_rows == 0 or n_cand == 0, which validates, writes *loss = 0, launches
 * nothing else and returns 0.
 * Errors before any launch: LGC_E_DIM (as lgc_dim_ok); LGC_E_INVAL (a null required pointer -- table, row_users, cand_items,
 * target, loss, grad_users, grad_cands, status --, exactly one of ign_ptr and ign_items, a negative n_rows, n_cand or
 * table_rows, size < 1, stride or grad_stride below dim, g_stride below n_cand, inv_tau not finite or <= 0, split outside
 * [0, table_rows]); LGC_E_RANGE (n_rows, n_cand or table_rows >= 2^31, or n_cand above 65535 * 128: the panel then stays
 * below 2^54 floats and the workspace arithmetic cannot overflow);
 * LGC_E_ALIGN (an fp32 or int32 pointer or the workspace not dword aligned, an int64 pointer not 8-byte aligned);
 * LGC_E_WORKSPACE (a workspace that is too small or missing).
 * ------------------------------------------------------------------------------------- */
size_t lgc_softmax_workspace_bytes(int64_t n_rows, int64_t n_cand);
int lgc_softmax_batch(const float *table, int64_t stride, int64_t table_rows, int64_t split, int32_t dim,
                      const int64_t *row_users, int64_t n_rows,
                      const int64_t *cand_items, int64_t n_cand,
                      const int32_t *target,
                      const int32_t *ign_ptr, const int64_t *ign_items,
                      const float *cand_bias,
                      float inv_tau, int64_t size,
                      float *loss, float *row_loss, int32_t *n_adm,
                      float *grad_logits, int64_t g_stride,
                      float *grad_users, float *grad_cands, int64_t grad_stride,
                      void *workspace, size_t workspace_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Cross-table retrieval (an addition to ABI 14: exports only): per query row of ONE table the k best rows of ANOTHER, with
 * a global eligibility mask, a per-query exclusion list and one skipped id per query -- "recommend, but never what is out of
 * stock and never what this user already bought" (user -> items), "which users should hear about this product" (item ->
 * users, its buyers left out) and lookalike users (user -> users).  Upstream's rule masked = score * (1 - seen) lets a seen
 * item compete with score 0; here it is REMOVED.  Scoring runs on the fp32 matrix cores and the selection in the same
 * launch, as in lgc_item_neighbors: no score is written to memory.
 *
 * lgc_retrieve_topk: per query the k best eligible candidates.
 *   queries    fp32 [n_query_rows, dim], rows query_stride floats apart; cands fp32 [n_cand, dim], rows cand_stride floats
 *              apart, n_cand >= 1.  Strides >= dim; columns at or past dim are never read.  The two tables may be the same
 *              memory
 *   query_ids  int64 [n_queries] rows of `queries`, any order, repeats allowed; NULL = query r is row r.  An id outside
 *              [0, n_query_rows) sets LGC_ST_INDEX_OOB in `status` and its whole result row is -1 / -inf; every id is
 *              range-checked before any address is formed from it
 *   query_scale, cand_scale  fp32 [n_query_rows] and [n_cand], both or neither (LGC_E_INVAL otherwise): s = (dot *
 *              query_scale[id]) * cand_scale[c], left to right, each product rounded, as in lgc_item_neighbors; without
 *              them s = dot
 *   cand_ok    uint8 [n_cand] or NULL: a candidate with cand_ok[c] == 0 is eligible for nobody
 *   list_ptr, list_items  the exclusion lists, a CSR: int64 [n_lists + 1] and int64 entries, candidate indices.  list_ptr
 *              is read on trust, as lgc_mask_topk and lgc_rank_positions read theirs.  list_ptr NULL = no lists (list_items
 *              and list_rows are then ignored).  A list is ascending (ingest.seen_csr, SeenLists.from_dense); an entry
 *              equal to its predecessor is harmless, an entry outside [0, n_cand) is ignored, an unsorted list gives an
 *              unspecified selection but never an access out of range.  A candidate in the query's list is REMOVED; there is
 *              no ZERO mode here (lgc_mask_topk and recommend_topk keep upstream's rule)
 *   list_rows  int64 [n_queries] or NULL: the list of query r is number list_rows[r], with NULL it is the query's id.  -1 =
 *              no list; any other value outside [0, n_lists) sets LGC_ST_INDEX_OOB and gives the row -1 / -inf -- a request
 *              whose filter cannot be found is not answered unfiltered
 *   skip_id    int64 [n_queries] or NULL: candidate skip_id[r] is not eligible for query r (the query's own row where both
 *              tables are one); -1 or any value outside the table skips nothing
 *   k          1 .. LGC_RETRIEVE_MAX_K
 *   slices     0 .. LGC_RETRIEVE_MAX_SLICES: the candidate table is cut into that many ranges of 128-row tiles, one workgroup
 *              per (64 queries, range), and a merge launch follows where there is more than one range; 0 = the library
 *              chooses (the smallest count that gives about 512 workgroups); a count above the number of candidate tiles is
 *              clamped to it.  The limit is not lgc_item_neighbors' 64: an audience request is one tile of queries over
 *              thousands of candidate tiles.  The result does not depend on it
 *   out_index  int64 [n_queries, k]; out_value fp32 [n_queries, k] or NULL.  With fewer than k eligible candidates the tail
 *              of the row is -1 / -inf
 *   workspace  device memory of at least lgc_retrieve_workspace_bytes(n_queries, n_cand, k, slices) bytes, 8-byte aligned:
 *              n_queries * (ranges in use) * k words of 8 bytes where there is more than one range; may be NULL where that is
 *              0.  The size function returns 0 for sizes the call would refuse and grows monotonically in n_queries, n_cand,
 *              k and in slices over 1 .. LGC_RETRIEVE_MAX_SLICES
 * Arithmetic: dot is lgc_score_rows' chain with the query row the first factor -- fused multiply-adds over d ascending from
 * +0, zeros past dim -- so it has that function's bits, except that a sum of -0 may come out as +0.
 * Order: lgc_mask_topk's total order -- every NaN first, then +inf, the finite values descending with -0 = +0, then -inf;
 * equal elements by ascending index.  It is strict, so the result depends neither on the tile shape nor on `slices` nor on
 * the order of arrival.  A NaN comes back as the quiet NaN 0x7FFFFFFF and -0 as +0.  No float atomics: the same bytes on
 * every run.
 * Errors before any launch, no output touched: LGC_E_DIM (as lgc_dim_ok); LGC_E_INVAL (a null required pointer -- queries,
 * cands, out_index, status --, a negative count, a stride below dim, one scale without the other, list_ptr without
 * list_items); LGC_E_RANGE (k or slices outside their ranges, n_cand < 1, n_queries, n_query_rows, n_cand or n_lists >=
 * 2^31 - 1); LGC_E_ALIGN (an fp32 pointer not dword aligned, an int64 pointer or the workspace not 8-byte aligned);
 * LGC_E_WORKSPACE (a workspace that is too small or missing).  n_queries == 0 validates, launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_RETRIEVE_MAX_K 64
#define LGC_RETRIEVE_MAX_SLICES 1024
size_t lgc_retrieve_workspace_bytes(int64_t n_queries, int64_t n_cand, int32_t k, int32_t slices);
int lgc_retrieve_topk(const float *queries, int64_t query_stride, int64_t n_query_rows,
                      const float *cands, int64_t cand_stride, int64_t n_cand, int32_t dim,
                      const int64_t *query_ids, int64_t n_queries,
                      const float *query_scale, const float *cand_scale,
                      const uint8_t *cand_ok,
                      const int64_t *list_ptr, const int64_t *list_items, const int64_t *list_rows, int64_t n_lists,
                      const int64_t *skip_id,
                      int32_t k, int32_t slices,
                      int64_t *out_index, float *out_value,
                      void *workspace, size_t workspace_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Bought together (an addition to ABI 14: exports only): per query ITEM the k items that share most buyers with it --
 * "customers who bought this also bought", the item-kNN baseline -- from the two purchase CSRs alone: no embedding, no
 * training.  Counting, scoring and selection are one launch per band of the catalogue; the counts live in LDS and only
 * those of the returned items are written out.
 *
 * lgc_cooccur_topk: per query item the k best eligible items.
 *   buyer_ptr, buyer_users  item -> users: int64 [n_items + 1] and int64 entries (BuyerLists); n_items >= 1
 *   seen_ptr, seen_items    user -> items: int64 [n_users + 1] and int64 entries (SeenLists, ingest.seen_csr)
 *              Both ptr arrays are read on trust, as lgc_mask_topk and lgc_retrieve_topk read theirs.  Every ENTRY is
 *              range-checked before an address is formed from it: a buyer outside [0, n_users) or an item outside
 *              [0, n_items) is skipped and sets LGC_ST_INDEX_OOB in `status`.  The lists are ascending and distinct, as
 *              BuyerLists and SeenLists build them.  A repeated entry counts as often as it occurs; an unsorted list gives
 *              unspecified counts but never an access out of range
 *   Count      for query item q and item j, c(q, j) = the sum over the entries u of q's buyer list of the number of entries of
 *              u's item list equal to j.  a = buyer_ptr[q + 1] - buyer_ptr[q] and b the same for j: list lengths in entries.
 *              Integer adds only (uint32 LDS atomics, whose order does not show); no float atomics anywhere: the same bytes on
 *              every run.  With distinct lists c <= a < 2^31 - 1; a count that repeated entries push past 2^32 - 1 wraps
 *   Eligible   item j is a candidate for q iff j != q, c >= min_count (min_count >= 1, LGC_E_RANGE otherwise: an item that
 *              shares no buyer is never returned) and item_ok is NULL or item_ok[j] != 0 (uint8 [n_items])
 *   Score      in fp32, every step rounded on its own (-ffp-contract=off), by `measure`:
 *              LGC_COOCCUR_COUNT    s = (float)c, round to nearest even
 *              LGC_COOCCUR_COSINE   ra = 1.0f / sqrtf((float)a), rb = 1.0f / sqrtf((float)b), the conversion, the root and the
 *                                   division each correctly rounded (lgc_build_csr's recipe for deg^-1/2);
 *                                   s = fl(fl((float)c * ra) * rb)
 *              LGC_COOCCUR_JACCARD  s = (float)c / (float)(a + b - c): the integer formed in int64 and converted once, the
 *                                   division correctly rounded.  With distinct lists the denominator is >= 1; where repeated
 *                                   entries make it <= 0 the candidate is not eligible
 *   Order      lgc_mask_topk's total order on (s, ascending j).  It is strict, so the result depends neither on `band` nor on
 *              the order of arrival
 *   query_ids  int64 [n_queries] items, any order, repeats allowed; NULL = query r is item r.  An id outside [0, n_items)
 *              sets LGC_ST_INDEX_OOB and its row is -1 / -inf / 0; it is range-checked before any address is formed from it
 *   k          1 .. LGC_COOCCUR_MAX_K
 *   band       the item counters one workgroup holds in LDS: the catalogue is cut into ceil(n_items / band) bands, one
 *              workgroup per (query, band), and a merge launch follows where there is more than one band.  0 = the library
 *              chooses (16384); an explicit value is a multiple of 64 in [64, LGC_COOCCUR_MAX_BAND],
 *              what the LDS budget allows (LGC_E_RANGE otherwise, as for a band that cuts the catalogue into more than 2^20
 *              bands).  A band wider than the catalogue holds the catalogue, rounded up to 64.  It exists so that tests can cross band edges on small catalogues; it never changes a result
 *   out_index  int64 [n_queries, k]; out_value fp32 [n_queries, k] or NULL; out_count int32 [n_queries, k] or NULL: the
 *              count c of each returned item (with several bands the merge launch counts the k returned items again: a place
 *              of the workspace has no room for a count).  A row with fewer than k candidates ends in -1 / -inf / 0
 *   workspace  device memory of at least lgc_cooccur_workspace_bytes(n_queries, n_items, k, band, stream) bytes, 8-byte aligned:
 *              n_queries * bands * k words of 8 bytes where there is more than one band, else 0; may be NULL where that is 0.
 *              The size function returns 0 for sizes the call would refuse and grows monotonically in n_queries, n_items, k.
 *              It takes the stream of the call it sizes, as every entry of this library that is not on the fixed list of
 *              host-only queries does; it runs on the host, enqueues nothing and reads nothing through the handle (NULL is
 *              fine): what it returns depends on its four sizes alone
 * Errors before any launch, no output touched: LGC_E_INVAL (a null required pointer -- the four list arrays, out_index,
 * status --, a negative n_queries or n_users, a measure that is none of the three); LGC_E_RANGE (k, band or min_count out of
 * range, n_items < 1, n_items, n_users or n_queries >= 2^31 - 1); LGC_E_ALIGN (an int64 pointer or the workspace not 8-byte
 * aligned, out_value, out_count or status not dword aligned); LGC_E_WORKSPACE (a workspace that is too small or missing).
 * n_queries == 0 validates, launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_COOCCUR_MAX_K 64
#define LGC_COOCCUR_MAX_BAND 32768
#define LGC_COOCCUR_COUNT   0
#define LGC_COOCCUR_COSINE  1
#define LGC_COOCCUR_JACCARD 2
size_t lgc_cooccur_workspace_bytes(int64_t n_queries, int64_t n_items, int32_t k, int32_t band, void *stream);
int lgc_cooccur_topk(const int64_t *buyer_ptr, const int64_t *buyer_users, int64_t n_items,
                     const int64_t *seen_ptr, const int64_t *seen_items, int64_t n_users,
                     const int64_t *query_ids, int64_t n_queries,
                     const uint8_t *item_ok, int32_t min_count, int32_t measure,
                     int32_t k, int32_t band,
                     int64_t *out_index, float *out_value, int32_t *out_count,
                     void *workspace, size_t workspace_bytes, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Item-kNN recommender (an addition to ABI 14: exports only): per BASKET -- a user's purchase list, a cart, a session -- the k
 * items with the best sum of neighbour similarities over the basket's items, from a [n_items, kn] neighbour table
 * (lgc_cooccur_topk over the whole catalogue, or lgc_item_neighbors).  Accumulation, removal and selection are one launch
 * per band of the catalogue; the scores live in LDS.  No embedding is read and there is no float atomic anywhere: the same
 * inputs give the same bytes on every run.
 *
 * lgc_knn_recommend: per query the k best eligible items.
 *   nbr_index, nbr_value  the neighbour table: int64 [n_items, kn] and fp32 of the same shape, rows nbr_stride >= kn
 *              elements apart in both arrays; kn in 1 .. LGC_KNN_MAX_NEIGHBORS, the width lgc_cooccur_topk and
 *              lgc_item_neighbors produce.  An entry -1 is an empty place and is ignored.  Any other index outside
 *              [0, n_items) is skipped and sets LGC_ST_INDEX_OOB in `status`; it is range-checked before an address is formed
 *              from it.  Elements at or past kn of a row are never read.  The valid indices of a row are distinct, as the two
 *              producers build them; a row that repeats an index gives an unspecified score for that candidate but never an
 *              access out of range
 *   list_ptr, list_items, list_weight  the baskets, a CSR: int64 [n_lists + 1], read on trust as lgc_mask_topk reads its own,
 *              and int64 item indices, in any order, repeats allowed; list_weight fp32 per entry or NULL.  A basket entry
 *              outside [0, n_items) is skipped and sets LGC_ST_INDEX_OOB
 *   list_rows  int64 [n_queries]: query r uses list list_rows[r]; NULL = query r uses list r, and then n_queries <= n_lists.
 *              A list number outside [0, n_lists) sets LGC_ST_INDEX_OOB and its row is -1 / -inf / 0
 *   Score      the score of candidate j starts at acc = +0.0f and votes = 0.  The basket's entries are taken in list order
 *              t = 0, 1, ..., i = list_items[t]: where row i of the table holds j at place p, term = nbr_value[i, p] without
 *              weights or fl(list_weight[t] * nbr_value[i, p]) with them, then acc = fl(acc + term) and votes += 1.  The
 *              product and the add are each rounded on their own (-ffp-contract=off), never fused.  A repeated basket entry
 *              contributes each time it occurs.  The sum order is the basket's, so every output has one right answer, bit for
 *              bit; NaN and infinities propagate as the additions give them
 *   Eligible   item j is a candidate iff votes >= min_votes (min_votes >= 1, LGC_E_RANGE otherwise: an item nobody voted
 *              for is never returned), item_ok is NULL or item_ok[j] != 0 (uint8 [n_items]), and, with exclude_basket != 0,
 *              j is no valid entry of the basket: such an item is REMOVED, as in lgc_retrieve_topk (there is no zero mode)
 *   Order      lgc_mask_topk's total order on (score, ascending j).  It is strict, so the result depends neither on `band` nor
 *              on the order of arrival.  A NaN score comes back as 0x7FFFFFFF and -0 as +0
 *   k          1 .. LGC_KNN_MAX_K
 *   band       as in lgc_cooccur_topk: the items one workgroup holds in LDS, one workgroup per (query, band) and a merge
 *              launch where there is more than one band.  0 = the library chooses (8192);
 *              an explicit value is a multiple of 64 in [64, LGC_KNN_MAX_BAND] (LGC_E_RANGE otherwise, as for a band that
 *              cuts the catalogue into more than 2^20 bands): a band costs 8 bytes per item, the accumulator and the votes.
 *              A band wider than the catalogue holds the catalogue, rounded up to 64.  It exists so that tests can cross band
 *              edges on small catalogues; it never changes a result
 *   out_index  int64 [n_queries, k]; out_value fp32 [n_queries, k] or NULL; out_votes int32 [n_queries, k] or NULL: the
 *              votes of each returned item.  A row with fewer than k candidates ends in -1 / -inf / 0
 *   workspace  device memory of at least lgc_knn_workspace_bytes(n_queries, n_items, k, band, stream) bytes, 8-byte aligned:
 *              n_queries * bands * k places of 12 bytes (the candidate word and its votes) where there is more than one band,
 *              else 0; may be NULL where that is 0.  The size function returns 0 for sizes the call would refuse and grows
 *              monotonically in n_queries, n_items, k.  It takes the stream of the call it sizes, runs on the host, enqueues
 *              nothing and reads nothing through the handle (NULL is fine)
 * Errors before any launch, no output touched: LGC_E_INVAL (a null required pointer -- nbr_index, nbr_value, list_ptr,
 * list_items, out_index, status --, a negative n_queries or n_lists, nbr_stride < kn); LGC_E_RANGE (k, kn, band or min_votes
 * out of range, n_items < 1, n_items, n_lists or n_queries >= 2^31 - 1, list_rows NULL with n_queries > n_lists); LGC_E_ALIGN
 * (an int64 pointer or the workspace not 8-byte aligned, an fp32 or int32 pointer not dword aligned); LGC_E_WORKSPACE (a
 * workspace that is too small or missing).  n_queries == 0 validates, launches nothing and returns 0.
 * ------------------------------------------------------------------------------------- */
#define LGC_KNN_MAX_K 64
#define LGC_KNN_MAX_NEIGHBORS 64
#define LGC_KNN_MAX_BAND 16384
size_t lgc_knn_workspace_bytes(int64_t n_queries, int64_t n_items, int32_t k, int32_t band, void *stream);
int lgc_knn_recommend(const int64_t *nbr_index, const float *nbr_value, int64_t nbr_stride, int64_t n_items, int32_t kn,
                      const int64_t *list_ptr, const int64_t *list_items, const float *list_weight, int64_t n_lists,
                      const int64_t *list_rows, int64_t n_queries,
                      const uint8_t *item_ok, int32_t exclude_basket, int32_t min_votes,
                      int32_t k, int32_t band,
                      int64_t *out_index, float *out_value, int32_t *out_votes,
                      void *workspace, size_t workspace_bytes, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGCONV_HIP_H */
