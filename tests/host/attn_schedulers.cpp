// Host check of the training attention's launch schedulers (csrc/vf_common.h): vf_attn_block_order hands every backward launch the permutation
// it runs its owner blocks in, vf_attn_query_groups decides which query views a forward workgroup serves.  A block listed twice or not at all
// is a silently missing or doubly written block of rows.  Stand-alone: built for the host with AddressSanitizer + UBSan and run as a
// subprocess by tests/test_attention_kernels_ref_host.py; never loaded into python, never run on a GPU.
//
// Grid: nviews 1..64, twin -32..64, by_key 0 / 1, vpb = 2 (the backward kernels: 128-row owner blocks of 64-token views).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../viewformer_amd/csrc/vf_common.h"

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (++failures <= 20) {                           \
                std::fprintf(stderr, "FAIL %s: ", #cond);     \
                std::fprintf(stderr, __VA_ARGS__);            \
                std::fprintf(stderr, "\n");                   \
            }                                                 \
        }                                                     \
    } while (0)

// weight of owner block b recomputed from vf_attn_visible alone: streamed views t of which some owner view of the block is a partner
static int block_weight(int nviews, int vpb, int b, int twin, bool by_key) {
    int cnt = 0;
    for (int t = 0; t < nviews; ++t) {
        bool any = false;
        for (int v = b * vpb; v < (b + 1) * vpb && v < nviews; ++v) any = any || (by_key ? vf_attn_visible(t, v, twin) : vf_attn_visible(v, t, twin));
        cnt += any ? 1 : 0;
    }
    return cnt;
}

static void check_block_order(int nviews, int twin, bool by_key) {
    const int vpb = 2, nblocks = (nviews + vpb - 1) / vpb;
    const vf_attn_order o = vf_attn_block_order(nviews, vpb, nblocks, twin, by_key);
    int seen[64];
    std::memset(seen, 0, sizeof seen);
    for (int r = 0; r < nblocks; ++r) {
        const int b = o.blk[r];
        CHECK(b < nblocks, "nviews %d twin %d by_key %d: rank %d holds block %d of %d", nviews, twin, (int)by_key, r, b, nblocks);
        if (b < nblocks) ++seen[b];
    }
    for (int b = 0; b < nblocks; ++b) CHECK(seen[b] == 1, "nviews %d twin %d by_key %d: block %d listed %d times", nviews, twin, (int)by_key, b, seen[b]);
    for (int r = 0; r + 1 < nblocks; ++r) {
        const int a = o.blk[r], b = o.blk[r + 1];
        if (a >= nblocks || b >= nblocks) continue;
        const int wa = block_weight(nviews, vpb, a, twin, by_key), wb = block_weight(nviews, vpb, b, twin, by_key);
        CHECK(wa > wb || (wa == wb && a < b), "nviews %d twin %d by_key %d: rank %d block %d (weight %d) before block %d (weight %d)", nviews, twin,
              (int)by_key, r, a, wa, b, wb);
    }
    for (int r = nblocks; r < 64; ++r) CHECK(o.blk[r] == r, "nviews %d twin %d: the unused rank %d holds %d", nviews, twin, r, (int)o.blk[r]);
}

static unsigned long long group_union(const vf_attn_groups& g, int b, int nviews, int twin) {
    unsigned long long m = 0ull;
    for (int j = 0; j < 4; ++j) {
        const int v = g.view[b][j];
        if (v == 0xFF) continue;
        for (int t = 0; t < nviews; ++t)
            if (vf_attn_visible(v, t, twin)) m |= 1ull << t;
    }
    return m;
}

static int popcount64(unsigned long long m) {
    int c = 0;
    for (; m; m &= m - 1) ++c;
    return c;
}

static void check_query_groups(int nviews, int twin) {
    const vf_attn_groups g = vf_attn_query_groups(nviews, twin);
    CHECK(g.n >= 1 && g.n <= 64, "nviews %d twin %d: %d groups", nviews, twin, g.n);
    if (g.n < 1 || g.n > 64) return;
    int seen[64];
    std::memset(seen, 0, sizeof seen);
    for (int b = 0; b < g.n; ++b)
        for (int j = 0; j < 4; ++j) {
            const int v = g.view[b][j];
            if (v == 0xFF) continue;
            CHECK(v < nviews, "nviews %d twin %d: group %d holds view %d", nviews, twin, b, v);
            if (v < nviews) ++seen[v];
        }
    for (int v = 0; v < nviews; ++v) CHECK(seen[v] == 1, "nviews %d twin %d: view %d served %d times", nviews, twin, v, seen[v]);
    for (int b = g.n; b < 64; ++b)
        for (int j = 0; j < 4; ++j) CHECK(g.view[b][j] == 0xFF, "nviews %d twin %d: the unused group %d holds a view", nviews, twin, b);
    // vf_attn_groups holds the views only, no union of its own: the key views a group walks are recomputed here from vf_attn_visible, every
    // group must see something, and the groups come by descending size of that union
    int prev = 1 << 30;
    for (int b = 0; b < g.n; ++b) {
        const unsigned long long uni = group_union(g, b, nviews, twin);
        const int w = popcount64(uni);
        CHECK(w >= 1, "nviews %d twin %d: group %d sees nothing", nviews, twin, b);
        CHECK(w <= prev, "nviews %d twin %d: group %d (weight %d) after a group of weight %d", nviews, twin, b, w, prev);
        prev = w;
    }
}

// vf_attn_visible against the definition written out (include/vf_hip.h): every view sees itself; plain: kv <= qv; twin Vc: kv < min(qv, Vc);
// streams Sv: the sequence is block-causal, a branch view (s, i) sees the sequence's views below i
static bool visible_def(int qv, int kv, int twin) {
    if (kv == qv) return true;
    if (twin <= -2) {
        const int Sv = -twin;
        if (kv / Sv != 0) return false;
        return qv / Sv == 0 ? kv < qv : kv % Sv < qv % Sv;
    }
    if (twin == -1) return kv < qv;
    return kv < twin && kv < qv;
}

int main() {
    long cells = 0;
    for (int nviews = 1; nviews <= 64; ++nviews)
        for (int twin = -32; twin <= 64; ++twin) {
            for (int q = 0; q < nviews; ++q)
                for (int k = 0; k < nviews; ++k)
                    CHECK(vf_attn_visible(q, k, twin) == visible_def(q, k, twin), "visible(%d, %d, twin %d)", q, k, twin);
            check_block_order(nviews, twin, false);
            check_block_order(nviews, twin, true);
            check_query_groups(nviews, twin);
            cells += 2;
        }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("attention schedulers: %ld (nviews, twin, by_key) cells clean\n", cells);
    return 0;
}
