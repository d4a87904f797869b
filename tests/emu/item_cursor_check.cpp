// item_cursor_check.cpp — the proof behind csrc/items.h, by brute force: on every (item width, extra, T, length table, grid) below, the
// walks of the persistent kernels through ItemCursor visit every item that has work exactly once, with exactly the fields a
// row-by-row enumeration gives.  A stand-alone program (tests/test_item_cursor.py builds it with the sanitizers and runs it):
//   check one  the grid-stride walk w, w + W, ... through decode(), in the order item_order_rule grants a request for XCD-major
//              (k_rb_conv, k_rb_conv_pw, k_ups_pl, k_ups64; with the look-ahead decode of the next item those kernels do);
//   check two  k_mrf_p's walk: min(W, 8) groups, each group's contiguous share, stride = the group's workgroups, advance() on a
//              copy of the cursor for the next item;
//   and wherever the rule grants XCD-major, every workgroup's remapped indices strictly increase.
// The host's count (valid_items / item_launch) must agree with the enumeration as well.
#include <cstdio>
#include <set>
#include <vector>

#include "items.h"
#include "kernels.h"

using namespace m355;

namespace {
long n_walks = 0, n_items = 0;
int fails = 0;

void fail(const char* what, int N, int extra, int T, const std::vector<int>& len, int W, int w, int it) {
    if (++fails > 20) return;
    fprintf(stderr, "FAIL %s: N %d extra %d T %d W %d workgroup %d item %d lengths", what, N, extra, T, W, w, it);
    for (int l : len) fprintf(stderr, " %d", l);
    fprintf(stderr, "\n");
}

bool same(const RowItem& a, const RowItem& b) { return a.b == b.b && a.t0 == b.t0 && a.len == b.len && a.last == b.last; }

template <int N, int EXTRA>
void check_table(int T, const std::vector<int>& len, const std::vector<int>& grids) {
    const int B = (int)len.size();
    // the list, row by row: a row of min(len, T) > 0 positions (+ EXTRA) in blocks of N
    std::vector<RowItem> list;
    for (int b = 0; b < B; ++b) {
        const int l = len[b] > T ? T : len[b];
        if (l <= 0) continue;
        for (int t0 = 0; t0 < l + EXTRA; t0 += N) list.push_back(RowItem{b, t0, l, l - 1});
    }
    const int nitems = (int)list.size();
    if (valid_items(len.data(), len.data(), B, T + EXTRA, N, EXTRA) != nitems) fail("valid_items", N, EXTRA, T, len, 0, 0, nitems);
    const RowLenSc reader{len.data(), T};

    for (int W : grids) {
        const ItemLaunch il = item_launch(len.data(), len.data(), B, T + EXTRA, N, EXTRA, W, 1);
        if (il.nvalid != nitems || il.grid != (nitems < W ? nitems : W) || il.item_order != item_order_rule(1, nitems, il.grid))
            fail("item_launch", N, EXTRA, T, len, W, 0, nitems);

        // ---- check one: grid stride through decode()
        const int order = item_order_rule(1, nitems, W);
        std::vector<int> seen((size_t)nitems, 0);
        for (int w = 0; w < W && w < nitems; ++w) {
            ItemCursor<N, EXTRA> cur(reader, B, nitems, order);
            int prev = -1;
            for (int it = w; it < nitems; it += W) {
                const int e = xcd_major(it, nitems, order);
                if (e < 0 || e >= nitems) { fail("remap out of range", N, EXTRA, T, len, W, w, it); break; }
                if (order && e <= prev) fail("XCD-major indices do not grow", N, EXTRA, T, len, W, w, it);
                prev = e;
                if (!same(cur.decode(it), list[(size_t)e])) fail("decode", N, EXTRA, T, len, W, w, it);
                ++seen[(size_t)e];
                const int itn = it + W < nitems ? it + W : it;  // the kernels decode the next item while they work on this one
                if (!same(cur.decode(itn), list[(size_t)xcd_major(itn, nitems, order)])) fail("decode (next item)", N, EXTRA, T, len, W, w, itn);
                ++n_items;
            }
        }
        for (int e = 0; e < nitems; ++e)
            if (seen[(size_t)e] != 1) fail("grid stride: item not visited exactly once", N, EXTRA, T, len, W, -1, e);

        // ---- check two: k_mrf_p's walk
        std::fill(seen.begin(), seen.end(), 0);
        const int nblk = W, ngrp = nblk < 8 ? nblk : 8;
        for (int w = 0; w < W; ++w) {
            const int xcd = w % ngrp, slot = w / ngrp;
            const int per_xcd = (nitems + ngrp - 1) / ngrp, nslot = (nblk + ngrp - 1 - xcd) / ngrp;
            const int item_end = (xcd + 1) * per_xcd < nitems ? (xcd + 1) * per_xcd : nitems;
            int item = xcd * per_xcd + slot;
            ItemCursor<N, EXTRA> cur(reader, B, nitems, 0);
            if (item < item_end) cur.advance(item);
            for (int item_next = item; item < item_end; item = item_next) {
                const int l = reader(cur.r);
                const RowItem got{cur.r, (item - cur.base) * N, l, l > 0 ? l - 1 : 0};
                if (!same(got, list[(size_t)item])) fail("advance", N, EXTRA, T, len, W, w, item);
                ++seen[(size_t)item];
                item_next = item + nslot;
                ItemCursor<N, EXTRA> cn = cur;
                if (item_next < item_end) cn.advance(item_next);
                cur = cn;
                ++n_items;
            }
        }
        for (int e = 0; e < nitems; ++e)
            if (seen[(size_t)e] != 1) fail("contiguous eighths: item not visited exactly once", N, EXTRA, T, len, W, -1, e);
        n_walks += 2;
    }
}

template <int N, int EXTRA>
void check_width() {
    std::vector<int> grids;
    for (int W = 1; W <= 24; ++W) grids.push_back(W);
    grids.push_back(32);
    grids.push_back(100);
    grids.push_back(256);
    unsigned rng = 12345u + 977u * (unsigned)N + (unsigned)EXTRA;
    auto draw = [&](unsigned n) {
        rng = rng * 1664525u + 1013904223u;
        return (rng >> 8) % n;
    };
    for (int T : {1, N - 1, N, N + 1, 260}) {
        const std::set<int> vs = {0, 1, N - 1, N, N + 1, T - 1, T, T + 5};  // lengths above T are clamped by the reader
        const std::vector<int> vals(vs.begin(), vs.end());
        const unsigned nv = (unsigned)vals.size();
        for (int rows = 1; rows <= 9; ++rows) {
            std::vector<std::vector<int>> tables;
            for (int v : vals) tables.emplace_back((size_t)rows, v);  // every row the same length (all rows empty among them)
            for (int hole = 0; hole < 3; ++hole) {                     // empty rows first, in the middle, last; the others cycle through the set
                std::vector<int> t((size_t)rows);
                for (int b = 0; b < rows; ++b) t[(size_t)b] = vals[1 + (size_t)(b + hole) % (nv - 1)];
                const int at = hole == 0 ? 0 : (hole == 1 ? rows / 2 : rows - 1);
                t[(size_t)at] = 0;
                if (rows > 3) t[(size_t)(at + 1 < rows ? at + 1 : at - 1)] = 0;  // two empty rows in a row
                tables.push_back(t);
            }
            for (int k = 0; k < 5; ++k) {  // random draws from the set
                std::vector<int> t((size_t)rows);
                for (int& x : t) x = vals[draw(nv)];
                tables.push_back(t);
            }
            for (const auto& t : tables) check_table<N, EXTRA>(T, t, grids);
        }
    }
}
}  // namespace

int main() {
    check_width<31, 0>();
    check_width<31, 1>();
    check_width<32, 0>();
    check_width<32, 1>();
    check_width<127, 0>();
    check_width<127, 1>();
    check_width<128, 0>();
    check_width<128, 1>();
    printf("item cursor: %ld walks, %ld items, %d failures\n", n_walks, n_items, fails);
    return fails ? 1 : 0;
}
