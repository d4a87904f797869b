// items.h — the work items of the persistent decoder kernels on a ragged batch (k_mrf_p, k_rb_conv, k_rb_conv_pw, k_ups_pl,
// k_ups64): which items exist, in which order a workgroup takes them, how an index becomes (row, first column, length), and how
// the launcher sizes the grid.  This is the one place for that decision; a kernel that adopts the cursor inherits the proof in
// tests/emu/item_cursor_check.cpp.
//
// Which items exist.  A row b of a batch has len_b <= T positions and is cut into blocks of N: an item is a (row, block) pair that
// HAS work, row b contributes nv_b = ceil((len_b + EXTRA) / N) of them (0 for an empty row; EXTRA = 1 for the polyphase
// upsamplers, where len input positions give len + 1 output positions).  A block that starts at or past its row's length is never
// computed: its output columns are past the row's end, every consumer masks its input at the row's length, and the workspace is
// zero-filled when it is allocated — so a batch costs the sum of its rows' lengths, not rows x the longest (ragged batches, round 6).
// Valid items are numbered row by row, 0 .. nvalid - 1; the launcher counts them from the host's copy of the lengths (valid_items).
//
// How an index becomes an item.  A cursor (row, first valid index of that row, the row's count) is advanced until the index falls
// into its row.  It ONLY MOVES FORWARD — a workgroup decodes indices that grow, so an item costs the rows passed since the last one,
// not a search — and that is the one rule every walk below must keep.  (An index is < nvalid, so the walk ends inside the batch; the
// row bound guards a count that disagrees with the table.)
//
// In which order.  Workgroup w of a grid of W runs on XCD w % 8.
//   * grid stride (k_rb_conv, k_rb_conv_pw, k_ups_pl, k_ups64): w takes the logical items w, w + W, w + 2 W, ...  Taken literally
//     (order 0), consecutive items of a row — which share their halo columns, or (k_ups64: 127-position items) the 128-byte lines
//     their rows' ends fall into — land on eight different XCDs and are fetched from HBM by each of them.  XCD-major (order 1):
//     logical item 8 q + x becomes the q-th item of XCD x's contiguous eighth of the items (xcd_major: a bijection for every item
//     count), so that the 32 CUs of an XCD work on neighbouring items at the same time and the shared bytes come out of that XCD's
//     L2.  The remapped indices of a workgroup must still grow: they do when W % 8 == 0 or W == the item count, and ONLY then
//     (item_order_rule); on any other grid the cursor would skip whole rows' items, so such a launch walks in order 0.
//   * contiguous eighths (k_mrf_p, since round 3): the workgroups form min(W, 8) groups, group x owns the x-th contiguous share of
//     ceil(nvalid / groups) items and its workgroups stride through it — the same locality without a remap, increasing by
//     construction; the shares hold equal numbers of VALID items whatever the rows' lengths.  It uses advance() directly.
#pragma once
#include "hipx.h"

namespace m355 {

// ---------------------------------------------------------------------------------------------------------------- device half
// a row's length through the scalar cache (s_load_dword: the constant address space tells hipcc that the table is read-only; as a
// plain global load it costs the item loop a vmcnt(0) — every prefetch drained — and one exposed round trip per item)
__device__ __forceinline__ int row_len_sc(const int* len, int b) {
#ifdef MI355_EMU
    return len[b];
#else
    typedef const int __attribute__((address_space(4))) * cptr_t;
    return ((cptr_t)(len))[b];
#endif
}

// how a cursor reads a row's length, clamped to the tensor's extent `cap`: through the scalar cache; the table is always there
struct RowLenSc {
    const int* len;
    int cap;
    __device__ __forceinline__ int operator()(int b) const {
        int ln = row_len_sc(len, b);
        if (ln > cap) ln = cap;
        return ln;
    }
};
// (any callable b -> clamped length will do: k_mrf_p brings its own, a plain load with "no table = full rows")

struct RowItem { int b, t0, len, last; };  // row, first position, the row's length (clamped) and its last valid position (0 for an empty row)

// logical item `it` of `n` -> the item it stands for (order 0: itself)
__device__ __forceinline__ int xcd_major(int it, int n, int order) {
    if (!order) return it;
    const int x = it & 7, q = it >> 3, f = n >> 3, rm = n & 7;
    return x * f + (x < rm ? x : rm) + q;
}

// N = positions per item, EXTRA = positions a row has beyond its length, Len = how the length table is read
template <int N, int EXTRA = 0, typename Len = RowLenSc>
struct ItemCursor {
    Len len;
    int B, nitems, order;
    int r, base, nv;  // the row, the valid index of its first item, its item count

    __device__ __forceinline__ ItemCursor(Len len_, int B_, int nitems_, int order_) : len(len_), B(B_), nitems(nitems_), order(order_), r(0), base(0), nv(0) {
        nv = count(0);
    }
    __device__ __forceinline__ int count(int b) const {
        const int ln = len(b);
        return ln > 0 ? (ln + EXTRA + N - 1) / N : 0;
    }
    // forward to the row that holds valid index v (v >= every index this cursor was advanced to before)
    __device__ __forceinline__ void advance(int v) {
        while (v >= base + nv && r + 1 < B) {
            base += nv;
            ++r;
            nv = count(r);
        }
        r = WAVE_UNIFORM(r);
        base = WAVE_UNIFORM(base);
        nv = WAVE_UNIFORM(nv);
    }
    // logical item `it` of a grid-stride walk
    __device__ __forceinline__ RowItem decode(int it) {
        RowItem o;
        it = xcd_major(it, nitems, order);
        advance(it);
        o.b = r;
        o.t0 = WAVE_UNIFORM((it - base) * N);
        o.len = len(o.b);
        o.last = o.len > 0 ? o.len - 1 : 0;
        return o;
    }
};

// ------------------------------------------------------------------------------------------------------------------ host half
// the item order a launch of `grid` persistent workgroups over `nitems` items may use: XCD-major only where every workgroup's
// sequence w, w + W, ... stays increasing after xcd_major
inline int item_order_rule(int order, long nitems, int grid) { return grid % 8 == 0 || grid == nitems ? order : 0; }

// what a launcher of a persistent kernel needs: the items with work, one workgroup per CU at most, the order that grid may use
struct ItemLaunch { int nvalid, grid, item_order; };
// lengths as for valid_items (kernels.h); N, extra as above; cus = current_device_cu_count(); order = the order asked for
ItemLaunch item_launch(const int* len_host, const int* len_dev, int B, int T, int N, int extra, int cus, int order);

}  // namespace m355
