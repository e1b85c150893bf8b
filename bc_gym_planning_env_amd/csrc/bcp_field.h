// bcp_field.h -- what is derived from the caller's maps and paths when they are bound or refreshed: the distance field of
// the lethal cells and its 1-bit tiles (the kernels are here, and the methods of their owner, DistanceField), and the
// launchers of the bitmap / path-table kernels of bcp_raster.h and bcp_step.h for a selection of entries.  The shapes come
// from bcp_field_plan.h.  Included by bcplan.hip after bcp_host.h.
#pragma once

// ---- Euclidean distance transform of the lethal cells over the padded map(s) (classify(), bcp_coop.h) ----------
// Distances are only ever compared with thresholds <= `clamp`, so the transform is exact up to `clamp` and
// saturates there.  pass 1: per padded column, vertical distance to the nearest lethal cell of that column.
__device__ __forceinline__ void edt_column(const uint32_t* __restrict__ bits, int64_t m, int cp, int rows, int cols, int wpr,
                                           int pad, int clamp, uint8_t* __restrict__ g)
{
    const int W = cols + 2 * pad, H = rows + 2 * pad;
    const int c = cp - pad;
    const uint32_t* mb = bits + m * (int64_t)rows * wpr;
    uint8_t* mg = g + m * (int64_t)W * H;
    const bool in_cols = c >= 0 && c < cols;
    int d = clamp;
    for (int rp = 0; rp < H; ++rp) {  // downward sweep
        const int r = rp - pad;
        const bool leth = in_cols && r >= 0 && r < rows && ((mb[r * wpr + (c >> 5)] >> (c & 31)) & 1u);
        d = leth ? 0 : min(d + 1, clamp);
        mg[rp * W + cp] = (uint8_t)d;
    }
    d = clamp;
    for (int rp = H - 1; rp >= 0; --rp) {  // upward sweep
        const int r = rp - pad;
        const bool leth = in_cols && r >= 0 && r < rows && ((mb[r * wpr + (c >> 5)] >> (c & 31)) & 1u);
        d = leth ? 0 : min(d + 1, clamp);
        mg[rp * W + cp] = (uint8_t)min((int)mg[rp * W + cp], d);
    }
}

__global__ void edt_columns_kernel(const uint32_t* __restrict__ bits, EntrySelect sel, int rows, int cols, int wpr, int pad,
                                   int clamp, uint8_t* __restrict__ g)
{
    const int W = cols + 2 * pad;
    const int64_t total = sel.size() * W;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x)
        edt_column(bits, sel.entry(t / W), (int)(t % W), rows, cols, wpr, pad, clamp, g);
}

// pass 2: d^2(r,c) = min over |c - c'| < clamp of (c - c')^2 + g(r,c')^2, stored as floor(min(clamp, d)).
__device__ __forceinline__ void edt_cell(const uint8_t* __restrict__ g, int64_t idx, int W, int clamp, uint8_t* __restrict__ out)
{
    const int cp = (int)(idx % W);
    const uint8_t* row = g + (idx - cp);
    int best = clamp * clamp;
    const int lo = max(0, cp - clamp + 1), hi = min(W - 1, cp + clamp - 1);
    for (int k = lo; k <= hi; ++k) {
        const int gv = row[k];
        const int dd = (cp - k) * (cp - k) + gv * gv;
        best = dd < best ? dd : best;
    }
    int sq = (int)sqrt((double)best);
    while (sq * sq > best) --sq;
    while ((sq + 1) * (sq + 1) <= best) ++sq;
    out[idx] = (uint8_t)min(sq, clamp);
}

__global__ void edt_rows_kernel(const uint8_t* __restrict__ g, EntrySelect sel, int W, int H, int clamp,
                                uint8_t* __restrict__ out)
{
    const int64_t per = (int64_t)W * H, total = sel.size() * per;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x)
        edt_cell(g, sel.entry(it / per) * per + it % per, W, clamp, out);
}

// The distance field as one bit per cell, "a lethal cell is closer than t_out", in 32 x 32-cell tiles (CullDesc::near):
// all the outer test of the step asks.  One thread per output word = 32 consecutive cells of one row.
typedef uint32_t __attribute__((aligned(1))) EdtUnalignedWord;
__global__ void near_tiles_kernel(const uint8_t* __restrict__ edt, EntrySelect sel, int W, int H, int tiles_x, int tiles_y,
                                  int t_out, uint32_t* __restrict__ tiles)
{
    const int64_t per = (int64_t)tiles_x * tiles_y * 32, total = sel.size() * per;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        const int tx = (int)(it % tiles_x);
        const int64_t t = it / tiles_x;
        const int y = (int)(t % (tiles_y * 32));
        const int64_t e = sel.entry(t / (tiles_y * 32));
        uint32_t word = 0;
        if (y < H) {
            const uint8_t* row = edt + (e * H + y) * (int64_t)W + tx * 32;
            if (tx * 32 + 32 <= W) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t four = *reinterpret_cast<const EdtUnalignedWord*>(row + 4 * k);
#pragma unroll
                    for (int j = 0; j < 4; ++j) word |= (uint32_t)((int)((four >> (8 * j)) & 255u) < t_out) << (4 * k + j);
                }
            } else {
                for (int j = 0; tx * 32 + j < W; ++j) word |= (uint32_t)((int)row[j] < t_out) << j;
            }
        }
        tiles[e * per + ((int64_t)(y >> 5) * tiles_x + tx) * 32 + (y & 31)] = word;
    }
}

// CullDesc::step_near: the tiles at 1 / 2^shift of the resolution, a bit = the OR of the 2^shift x 2^shift bits it stands
// for.  One thread per output word: 2^shift rows of 2^shift neighbouring tiles, OR-ed and squeezed.
__global__ void near_coarsen_kernel(const uint32_t* __restrict__ tiles, EntrySelect sel, int tiles_x, int tiles_y, int shift,
                                    int ctx, int cty, uint32_t* __restrict__ coarse)
{
    const int64_t per = (int64_t)tiles_x * tiles_y * 32, cper = (int64_t)ctx * cty * 32, total = sel.size() * cper;
    const int f = 1 << shift, bits_out = 32 >> shift;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = sel.entry(it / cper);
        const int k = (int)(it % cper);
        const int Y = (k / (32 * ctx)) * 32 + (k & 31), TX = (k >> 5) % ctx;   // coarse row, coarse tile column
        uint32_t word = 0;
        for (int part = 0; part < f; ++part) {          // fine tile column part of this coarse word
            const int tx = TX * f + part;
            uint32_t rows = 0;
            for (int dy = 0; dy < f; ++dy) {
                const int y = Y * f + dy;
                if (tx < tiles_x && y < tiles_y * 32) rows |= tiles[e * per + ((int64_t)(y >> 5) * tiles_x + tx) * 32 + (y & 31)];
            }
            uint32_t squeezed = 0;
            for (int b = 0; b < bits_out; ++b) squeezed |= (uint32_t)(((rows >> (b << shift)) & ((1u << f) - 1u)) != 0) << b;
            word |= squeezed << (part * bits_out);
        }
        coarse[e * cper + k] = word;
    }
}

// The same transform for maps that fit into LDS (every private / pool map), one workgroup per map, `clamp` <= 60:
//   pass 1: h(r, c) = distance to the nearest lethal cell of ROW r, from the row's bit mask with clz / ctz on the 64 bits
//           either side of c -- no sweep, every cell on its own; four cells per thread, packed into an LDS dword;
//   pass 2: d^2(r, c) = min over |r - r'| < clamp of (r - r')^2 + h(r', c)^2, rows taken from the centre outwards and
//           abandoned once (r - r')^2 alone reaches the best value so far.
// It computes the very min the two kernels above compute (the order of the two 1-D passes does not matter), from LDS
// instead of through the caches: ~20 x faster, which is what lets a pool be topped up between steps.
__device__ __forceinline__ uint32_t edt_row_word(LdsWords row, int wpr, int w) { return (w >= 0 && w < wpr) ? row[w] : 0u; }

// bit i = column start + i of the row (zero outside the map), i = 0 .. 63
__device__ __forceinline__ uint64_t edt_row_window(LdsWords row, int wpr, int start)
{
    const int w0 = start >> 5, sh = start & 31;   // (arithmetic shift: floor for negative starts)
    const uint64_t lo = ((uint64_t)edt_row_word(row, wpr, w0 + 1) << 32) | edt_row_word(row, wpr, w0);
    const uint64_t hi = edt_row_word(row, wpr, w0 + 2);
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

typedef unsigned short EdtU16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t __attribute__((aligned(1))) EdtU32Unaligned;

__device__ __forceinline__ EdtU16x2 edt_pair(uint32_t word, uint32_t selector)
{
    const uint32_t v = __builtin_amdgcn_perm(0u, word, selector);
    return __builtin_bit_cast(EdtU16x2, v);
}

__global__ void __launch_bounds__(256) edt_lds_kernel(const uint32_t* __restrict__ bits, EntrySelect sel, int rows, int cols,
                                                      int wpr, int pad, int clamp, uint8_t* __restrict__ out)
{
    const int W = cols + 2 * pad, H = rows + 2 * pad, Wq = (W + 3) / 4;
    const LdsU32 bm = (LdsU32)lds_dyn;   // [rows][wpr] lethal mask
    const LdsU32 hq = bm + rows * wpr;   // [H][Wq] h, four cells per dword
    __attribute__((address_space(3))) uint8_t* const isq =
        (__attribute__((address_space(3))) uint8_t*)(hq + H * Wq);   // [clamp^2 + 1] min(clamp, floor(sqrt(.)))
    const int tid = threadIdx.x;
    const uint32_t far4 = (uint32_t)clamp * 0x01010101u;
    const int64_t n_sel = sel.size();
    for (int v = tid; v <= clamp * clamp; v += 256) {
        int sq = (int)__builtin_amdgcn_sqrtf((float)v);   // v <= 3600: the fix-ups make it exact
        while (sq * sq > v) --sq;
        while ((sq + 1) * (sq + 1) <= v) ++sq;
        isq[v] = (uint8_t)min(sq, clamp);
    }
    for (int64_t k = blockIdx.x; k < n_sel; k += gridDim.x) {
        const int64_t m = sel.entry(k);
        __syncthreads();   // the previous map's pass 2 is done with the LDS
        for (int i = tid; i < rows * wpr; i += 256) bm[i] = bits[m * (int64_t)rows * wpr + i];
        __syncthreads();
        // (a wave per row, a lane per group of four cells: no divisions, and the four cells share their two windows)
        for (int rp = tid >> 6; rp < H; rp += 4) {
            const int r = rp - pad;
            for (int q = tid & 63; q < Wq; q += 64) {
                uint32_t packed = far4;
                if (r >= 0 && r < rows) {
                    const LdsWords row = (LdsWords)(bm + r * wpr);
                    const int c0 = q * 4 - pad;
                    // left: bit 63 = column c0, bit 63 - j = column c0 - j;  right: bit j = column c0 + j
                    const uint64_t left = edt_row_window(row, wpr, c0 - 63), right = edt_row_window(row, wpr, c0);
                    packed = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {   // the same two windows seen from column c0 + b (clamp <= 60)
                        const uint64_t lb = (left >> b) | (right << (63 - b)), rb = right >> b;
                        const int dr = rb ? (int)__builtin_ctzll(rb) : 64, dl = lb ? (int)__builtin_clzll(lb) : 64;
                        packed |= (uint32_t)min(min(dr, dl), clamp) << (8 * b);
                    }
                }
                hq[rp * Wq + q] = packed;
            }
        }
        __syncthreads();
        uint8_t* field = out + m * (int64_t)W * H;
        // (two cells per packed 16-bit operation: all values are <= 2 * clamp^2 <= 7200; the square roots come from a
        //  table; no early exit -- it would cost as much per round as the round itself)
        for (int rp = tid >> 6; rp < H; rp += 4) {
            for (int q = tid & 63; q < Wq; q += 64) {
                EdtU16x2 best_lo = {(unsigned short)(clamp * clamp), (unsigned short)(clamp * clamp)}, best_hi = best_lo;
                for (int d = 0; d < clamp; ++d) {
                    const unsigned short dd = (unsigned short)(d * d);
                    const EdtU16x2 dd2 = {dd, dd};
                    const uint32_t up = rp - d >= 0 ? hq[(rp - d) * Wq + q] : far4;
                    const uint32_t dn = rp + d < H ? hq[(rp + d) * Wq + q] : far4;
                    // bytes 0, 1 / 2, 3 of a dword, zero-extended to a pair of 16-bit values (v_perm_b32)
                    const EdtU16x2 h_lo = __builtin_elementwise_min(edt_pair(up, 0x0c010c00u), edt_pair(dn, 0x0c010c00u));
                    const EdtU16x2 h_hi = __builtin_elementwise_min(edt_pair(up, 0x0c030c02u), edt_pair(dn, 0x0c030c02u));
                    best_lo = __builtin_elementwise_min(best_lo, (EdtU16x2)(h_lo * h_lo + dd2));
                    best_hi = __builtin_elementwise_min(best_hi, (EdtU16x2)(h_hi * h_hi + dd2));
                }
                const uint32_t four = (uint32_t)isq[best_lo.x] | ((uint32_t)isq[best_lo.y] << 8) |
                                      ((uint32_t)isq[best_hi.x] << 16) | ((uint32_t)isq[best_hi.y] << 24);
                uint8_t* const dst = field + rp * W + q * 4;
                if (q * 4 + 3 < W) {
                    *reinterpret_cast<EdtU32Unaligned*>(dst) = four;
                } else {
                    for (int b = 0; q * 4 + b < W; ++b) dst[b] = (uint8_t)(four >> (8 * b));
                }
            }
        }
    }
}

// The 1-bit tiles WITHOUT the distance field: bit (x, y) = "a lethal cell lies within dx^2 + dy^2 < t_out^2" is the lethal
// mask dilated by a disc, and a disc is a stack of horizontal runs: with reach(w) = isqrt(t_out^2 - 1 - w^2),
//     near(x, y) = OR over |w| < t_out of  V_|w|(x + w, y),     V_w(x, y) = OR over |dy| <= reach(w) of lethal(x, y + dy).
// reach() grows as w shrinks, so one pass from w = t_out - 1 down to 0 ORs every row within reach into a 96-bit window
// exactly once and shifts the window by +-w: ~250 integer instructions per 32-cell output word against ~1200 of the
// distance transform + threshold (edt_lds_kernel + near_tiles_kernel), and no 16 KB uint8 field to write and read back.
// The bits are those of near_tiles_kernel by construction (floor(sqrt(D2)) < t_out  <=>  D2 <= t_out^2 - 1; the transform's
// windows are wider than t_out); tests/test_gpu_pool.py::test_near_tiles_by_dilation_vs_thresholded_field compares the two word for word.  What a pool refresh runs
// while the steps only read the tiles (step_local_kernel); the uint8 field of such entries is marked stale (ensure_fields).
// One workgroup per map; LDS: the padded lethal rows with a zero word either side and t_out - 1 zero rows above and below.
__global__ void __launch_bounds__(256) near_dilate_kernel(const uint32_t* __restrict__ bits, EntrySelect sel, int rows, int cols,
                                                          int wpr, int pad, int t_out, int W, int H, int tiles_x, int tiles_y,
                                                          uint32_t* __restrict__ tiles, uint8_t* __restrict__ stale)
{
    const LdsU32 P = (LdsU32)lds_dyn;
    const int tid = threadIdx.x;
    const int margin = t_out - 1, pitch = tiles_x + 2, Ht = tiles_y * 32, Hp = Ht + 2 * margin;
    const LdsU32 reach = P + Hp * pitch;   // [t_out]
    for (int w = tid; w < t_out; w += 256) {
        const int v = t_out * t_out - 1 - w * w;
        int sq = (int)__builtin_amdgcn_sqrtf((float)v);   // v < 1024: the fix-ups make it exact
        while (sq * sq > v) --sq;
        while ((sq + 1) * (sq + 1) <= v) ++sq;
        reach[w] = (uint32_t)sq;
    }
    const int64_t n_sel = sel.size(), per = (int64_t)tiles_x * tiles_y * 32;
    for (int64_t k = blockIdx.x; k < n_sel; k += gridDim.x) {
        const int64_t m = sel.entry(k);
        const uint32_t* mb = bits + m * (int64_t)rows * wpr;
        __syncthreads();   // the previous map's words are no longer read
        // P[yp][1 + kx] bit b = lethal(column 32 kx + b - pad, row yp - margin - pad); zero outside the map
        for (int i = tid; i < Hp * pitch; i += 256) {
            const int yp = i / pitch, kp = i - yp * pitch;
            const int r = yp - margin - pad, start = 32 * (kp - 1) - pad;
            uint32_t word = 0;
            if (r >= 0 && r < rows && kp >= 1 && kp <= tiles_x) {
                const int w0 = start >> 5, sh = start & 31;   // (arithmetic shift: floor for negative starts)
                const uint32_t lo = (w0 >= 0 && w0 < wpr) ? mb[r * wpr + w0] : 0u;
                const uint32_t hi = (w0 + 1 >= 0 && w0 + 1 < wpr) ? mb[r * wpr + w0 + 1] : 0u;
                word = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
                const int left = cols + pad - 32 * (kp - 1);   // columns >= cols are not part of the map
                word = left >= 32 ? word : (left > 0 ? word & ((1u << left) - 1u) : 0u);
            }
            P[i] = word;
        }
        __syncthreads();
        for (int i = tid; i < Ht * tiles_x; i += 256) {
            const int y = i / tiles_x, kx = i - y * tiles_x;
            const LdsU32 centre = P + (y + margin) * pitch + kx;   // words kx - 1, kx, kx + 1 of row y
            uint32_t a = 0, b = 0, c = 0, word = 0;
            int in = -1;
            for (int w = t_out - 1; w >= 0; --w) {
                const int need = (int)reach[w];
                while (in < need) {
                    ++in;
                    const LdsU32 up = centre - in * pitch, dn = centre + in * pitch;
                    a |= up[0] | dn[0];
                    b |= up[1] | dn[1];
                    c |= up[2] | dn[2];
                }
                word |= w ? (b << w) | (a >> (32 - w)) | (b >> w) | (c << (32 - w)) : b;
            }
            const int left = W - 32 * kx;   // near_tiles_kernel leaves cells outside the padded field clear
            word = (y < H) ? (left >= 32 ? word : (left > 0 ? word & ((1u << left) - 1u) : 0u)) : 0u;
            tiles[m * per + ((int64_t)(y >> 5) * tiles_x + kx) * 32 + (y & 31)] = word;
        }
        if (stale && tid == 0) stale[m] = 1;
    }
}

// entries whose uint8 distance field is stale (near_dilate_kernel ran for them) -> a list for edt_lds_kernel & co.
__global__ void stale_fields_list_kernel(uint8_t* __restrict__ stale, int64_t n, int32_t* __restrict__ list, int32_t* __restrict__ count)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        if (stale[e]) {
            stale[e] = 0;
            list[atomicAdd(count, 1)] = (int32_t)e;
        }
}

// Derived map data (1-bit lethal mask, distance field) and path data (cos/sin columns, bounding boxes, bucket index)
// of the selected entries; `max_entries` bounds sel.size() and only sizes the grids.
static void launch_pack_bitmap(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    const MapDesc& m = h->map;
    hipLaunchKernelGGL(pack_bitmap_kernel, dim3(stride_grid(max_entries * m.rows * m.wpr, 256, sel.list != nullptr)), dim3(256), 0, s, h->map_data,
                       h->bitmap.get(), h->map_tiles.get(), sel, m.rows, m.cols, m.wpr, h->map_valid_rows, h->map_valid_cols);
    // the cell lists of the sparse egocentric views follow the maps: all of them are rebuilt lazily after a re-bind
    // (sel.list == nullptr), the re-sampled entries of a pool refresh right here, in stream order
    if (sel.list) h->ego_cells.recount(h, sel, max_entries, s);
    else h->ego_cells.invalidate();
}

// ---- DistanceField (declared in bcp_host.h) --------------------------------------------------------------------
inline hipError_t DistanceField::reserve_marks(size_t entries)
{
    hipError_t e = stale.reserve(entries);
    if (e == hipSuccess) e = stale_list.reserve(entries + 1);
    if (e != hipSuccess) {   // (without the list there are no marks)
        (void)stale.reset();
        (void)stale_list.reset();
    }
    return e;
}

inline int DistanceField::bind(bcp_handle* h, const FieldPlan& f, hipStream_t s)
{
    plan = f;
    CullDesc& C = h->cull;
    C = f.cull;
    if (!f.field) return BCP_OK;   // (culling off: the geometry alone, every in-map pose is AMBIGUOUS)
    C.on = 0;                      // (until everything below stands)
    HIP_TRY(edt.reserve(f.n_edt));
    HIP_TRY(edt_col.reserve(f.n_edt_col));
    HIP_TRY(near.reserve(f.n_near));
    HIP_TRY(near_coarse.reserve(f.n_near_coarse));
    // the stale marks of tiles-only rebuilds: the caller rebuilds every field next, so none is stale
    lazy = false;
    if (f.n_stale) HIP_TRY(reserve_marks(f.n_stale));
    if (stale.get()) HIP_TRY(hipMemsetAsync(stale.get(), 0, stale.capacity(), s));
    C.edt = edt.get();
    C.near = near.get();
    C.step_near = f.cull.step_near_shift > 0 ? near_coarse.get() : near.get();
    C.on = f.cull.on;
    return BCP_OK;
}

inline bool DistanceField::bind_reads_tiles_only(const bcp_handle* h, const FieldPlan& f)
{
    const Tuning& t = h->tune;
    return !h->map.shared && f.n_maps >= 32 && t.fused && t.adaptive && f.cull.on && t.near_dilate == 1;
}

inline bool DistanceField::refresh_reads_tiles_only(const bcp_handle* h)
{
    return h->parking.slots() && h->tune.fused && h->tune.adaptive && h->cull.on;
}

inline void DistanceField::launch_near_tiles(EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    const CullDesc& C = plan.cull;
    hipLaunchKernelGGL(near_tiles_kernel, dim3(stride_grid(max_entries * C.near_words, 256, sel.list != nullptr)), dim3(256), 0, s,
                       edt.get(), sel, C.width, C.height, C.near_tx, plan.tiles_y, C.t_out, near.get());
}

// near_dilate_kernel serves these maps: radius within a word, rows + margins in LDS
inline size_t DistanceField::near_dilate_lds() const
{
    const CullDesc& C = plan.cull;
    if (C.t_out < 1 || C.t_out > 32 || C.pad < C.t_out - 1) return 0;
    const size_t bytes = ((size_t)(plan.tiles_y * 32 + 2 * (C.t_out - 1)) * (C.near_tx + 2) + C.t_out) * sizeof(uint32_t);
    return bytes <= 64 * 1024 ? bytes : 0;
}

inline void DistanceField::launch_near_dilate(bcp_handle* h, EntrySelect sel, int64_t max_entries, uint8_t* marks, hipStream_t s)
{
    const MapDesc& m = h->map;
    const CullDesc& C = plan.cull;
    const int64_t blocks = std::min<int64_t>(max_entries, sel.list ? 4096 : 16384);
    hipLaunchKernelGGL(near_dilate_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), near_dilate_lds(), s, h->bitmap.get(), sel,
                       m.rows, m.cols, m.wpr, C.pad, C.t_out, C.width, C.height, C.near_tx, plan.tiles_y, near.get(), marks);
}

inline void DistanceField::launch_edt(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    const MapDesc& m = h->map;
    const CullDesc& C = plan.cull;
    const size_t lds = ((size_t)m.rows * m.wpr + (size_t)C.height * ((C.width + 3) / 4)) * sizeof(uint32_t) +
                       (((size_t)C.clamp * C.clamp + 1 + 3) & ~(size_t)3);
    // (one workgroup per map: worth it from a few dozen maps on; a lone shared map keeps the two wide kernels)
    if (C.clamp <= 60 && lds <= kMaxDynamicLds && h->tune.edt_in_lds && max_entries >= 32) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(edt_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        const int64_t blocks = std::min<int64_t>(max_entries, sel.list ? 2048 : 16384);
        hipLaunchKernelGGL(edt_lds_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), lds, s, h->bitmap.get(), sel,
                           m.rows, m.cols, m.wpr, C.pad, C.clamp, edt.get());
        return;
    }
    hipLaunchKernelGGL(edt_columns_kernel, dim3(stride_grid(max_entries * C.width, 64, sel.list != nullptr)), dim3(64), 0, s, h->bitmap.get(), sel, m.rows,
                       m.cols, m.wpr, C.pad, C.clamp, edt_col.get());
    hipLaunchKernelGGL(edt_rows_kernel, dim3(stride_grid(max_entries * C.width * C.height, 256, sel.list != nullptr)), dim3(256), 0, s, edt_col.get(),
                       sel, C.width, C.height, C.clamp, edt.get());
}

inline void DistanceField::launch_near_coarse(EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    const CullDesc& C = plan.cull;
    if (C.step_near_shift == 0) return;
    hipLaunchKernelGGL(near_coarsen_kernel, dim3(stride_grid(max_entries * C.step_near_tx * plan.cty * 32, 256, sel.list != nullptr)), dim3(256),
                       0, s, near.get(), sel, C.near_tx, plan.tiles_y, C.step_near_shift, C.step_near_tx, plan.cty, near_coarse.get());
}

// `tiles_only`: the caller's consumers read nothing but the tiles (the single-launch step) -- when near_dilate_kernel can
// serve the maps, the uint8 field is left stale and marked so; ensure_fields() brings it up to date for whoever asks for it
// later.
inline int DistanceField::rebuild(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s, bool tiles_only)
{
    if (!h->cull.edt) return BCP_OK;   // (bound with culling off)
    const int32_t dilate = h->tune.near_dilate;
    if (tiles_only && dilate >= 1 && near_dilate_lds() && (int64_t)stale.capacity() >= n_slots(h)) {
        launch_near_dilate(h, sel, max_entries, stale.get(), s);
        launch_near_coarse(sel, max_entries, s);
        lazy = true;
        return BCP_OK;
    }
    launch_edt(h, sel, max_entries, s);
    launch_near_tiles(sel, max_entries, s);
    if (dilate == 2 && near_dilate_lds()) launch_near_dilate(h, sel, max_entries, nullptr, s);
    launch_near_coarse(sel, max_entries, s);
    return BCP_OK;
}

// (One scratch list per handle: the readers of the uint8 field of ONE handle must share a stream, like everything else a
// handle does -- include/bcplan.h, "a handle is not thread-safe".)
// Before anything reads the uint8 field (two-launch and single-kernel step forms, bcp_pose_collides,
// bcp_get_distance_field): the transform of the entries a tiles-only refresh has left stale, on the reader's stream.  An
// entry is marked at the end of its refresh, in the refresh's stream order, so a refresh still running on another stream
// is simply picked up by the next call; the flag stays up for as long as such refreshes may be in flight.
inline int DistanceField::ensure_fields(bcp_handle* h, hipStream_t s)
{
    if (!lazy || !h->cull.edt || !stale.get()) return BCP_OK;
    // Has every tiles-only refresh issued so far finished?  Then this pass leaves no stale field behind and later calls can
    // skip their three launches until the next such refresh (which raises the flag again).
    bool settled = true;   // (no refresh ever issued: the stale marks come from bcp_set_costmaps, in stream order)
    if (h->refresh_recorded) {
        settled = hipEventQuery(h->refresh_done.get()) == hipSuccess;
        if (!settled) (void)hipGetLastError();   // (hipErrorNotReady)
    }
    const int64_t entries = (int64_t)stale.capacity();
    int32_t* count = stale_list.get() + entries;
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(stale_fields_list_kernel, dim3(stride_grid(entries, 256)), dim3(256), 0, s, stale.get(), entries,
                       stale_list.get(), count);
    const EntrySelect sel = {stale_list.get(), count, entries};
    launch_edt(h, sel, entries, s);
    HIP_TRY(hipGetLastError());
    if (settled) lazy = false;
    return BCP_OK;
}

inline int DistanceField::copy_field(bcp_handle* h, int64_t first_entry, int64_t n_entries, uint8_t* out, hipStream_t s)
{
    BCP_TRY(ensure_fields(h, s));
    const size_t per = (size_t)plan.cull.width * plan.cull.height;
    HIP_TRY(hipMemcpyAsync(out, edt.get() + first_entry * per, n_entries * per, hipMemcpyDeviceToDevice, s));
    return BCP_OK;
}

inline int DistanceField::copy_near(int64_t first_entry, int64_t n_entries, uint32_t* out, hipStream_t s)
{
    const size_t per = (size_t)plan.cull.near_words;
    HIP_TRY(hipMemcpyAsync(out, near.get() + first_entry * per, n_entries * per * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return BCP_OK;
}

// the costmap origins into the path records of private paths (kBoxOrigin): needs both the costmaps and the paths
static void launch_world_records(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    if (!h->path_bbox.get() || h->path.shared || !h->map.bits) return;
    hipLaunchKernelGGL(world_record_kernel, dim3(stride_grid(max_entries, 256, sel.list != nullptr)), dim3(256), 0, s, sel,
                       h->map.origins, h->map.ox, h->map.oy, h->path_bbox.get());
}

static void launch_path_data(bcp_handle* h, EntrySelect sel, int64_t max_entries, hipStream_t s)
{
    const PathDesc& p = h->path;
    hipLaunchKernelGGL(path_bbox_kernel, dim3(stride_grid(max_entries, 256, sel.list != nullptr)), dim3(256), 0, s, h->path_src, p.lens, p.max_len,
                       sel, h->dev.sp_prune, p.shared ? kPathBuckets : kPathBucketsCompact, h->path_bbox.get());
    hipLaunchKernelGGL(path_trig_kernel, dim3(stride_grid(max_entries * p.max_len, 256, sel.list != nullptr)), dim3(256), 0, s, h->path_src, h->path5.get(),
                       p.shared ? nullptr : h->path_pre.get(), h->path_bbox.get(), sel, p.max_len);
    if (p.shared)
        hipLaunchKernelGGL(path_index_kernel, dim3(stride_grid(max_entries * 2 * kPathBuckets, 256, sel.list != nullptr)), dim3(256), 0, s, h->path_src,
                           p.lens, p.max_len, sel, h->dev.sp_prune, h->path_bbox.get(), h->path_index.get());
    else   // (private paths: compact tables inside the records)
        hipLaunchKernelGGL(path_index_compact_kernel, dim3(stride_grid(max_entries * 2 * kPathBucketsCompact, 256, sel.list != nullptr)), dim3(256), 0,
                           s, h->path_src, p.lens, p.max_len, sel, h->dev.sp_prune, h->path_bbox.get());
    launch_world_records(h, sel, max_entries, s);
}
