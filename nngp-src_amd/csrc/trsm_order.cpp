// The ticket order of the persistent blocked solves (trsm_tickets.hip), built on the host.
// List scheduling on `workers` simulated workgroups with rough item durations: an item enters the table when the simulation starts
// it, i.e. after everything it depends on has FINISHED there -- so every dependency has a lower ticket whatever the real timing is.
// Priority: earliest deadline first, the deadline of an item being the block column it feeds (diagonal chain items before the
// updates of the next block column).  Updates come in two shapes: a 2 x 2 group of tiles takes every finished block column that is
// waiting for it EXCEPT the two right before its own block, up to four at a time, as one 256 x 256 item (deep K where the chip is
// throughput-bound); the last two block columns before a tile's own -- the updates on or next to the dependency chain -- are applied
// tile by tile (128 x 128 items: four times the parallelism where only latency counts).  Tiles without a partner (odd row-tile count, odd tail)
// take all their updates as 128 x 128 items.
// merged: the chain update of a paired tile is a UW item (it waits for the split rows of the previous block B_J, not for X_J)
// nq > 1: the workers are nq pools (the XCDs) with a table each.  A pair of row tiles belongs to 8 / (pairs) pools -- its bulk items are
// dealt to them by column pair, its two chains to the first two -- so that everything that reads the split rows of X of one row pair
// (1 MB per block column, read by every column pair's item) runs behind ONE L2, in the order in which it becomes ready: the items of one
// block-column range over all column pairs are queued together and start together.  `queue_of` receives each item's pool; `out` stays
// the global start order (an item's dependencies all precede it there).
//
// The tables decide how panels are grouped per update item and therefore the bits of every solve: tests/golden/trsm_order_pins.json
// holds them.  What must not change: the sequence of pushes and pops on the two kinds of heap, the two comparison operators (Done
// orders by t alone: ties fall as the heap's history has it), and every floating-point expression as written, in double.
#include "trsm_order.h"

#include <algorithm>
#include <queue>

namespace nngp {

namespace {

// Simulated item durations in us, from the stamps of GPU runs: a split item; a 128 x 128 item = tile0 + stage per 32-wide k-block;
// a 256 x 256 item = big0 + bigstage per k-block.  Finish times are sums such as now + tile0 + stage * nk * avail: this file is
// compiled with -ffp-contract=off (Makefile), because contracted into FMAs they round differently, ties among the running items
// fall the other way and the tables change (measured: clang++ -O3 with its default -ffp-contract=on against the same text with off).
struct TkCostModel { double split, tile0, stage, big0, bigstage; };
constexpr TkCostModel kCost = {10.0, 14.0, 0.6, 24.0, 1.6};

struct Ready {
    int key, c, r, type, J;  // type IT_*
    bool operator<(const Ready& o) const {  // priority_queue: largest first -> invert
        if (key != o.key) return key > o.key;
        if (c != o.c) return c > o.c;
        if (r != o.r) return r > o.r;
        return type > o.type;
    }
};
struct Done {
    double t;
    int type, r, cq, J, npan;
    int q = 0;
    bool operator<(const Done& o) const { return t > o.t; }
};

class ListScheduler {
public:
    ListScheduler(int mt, int nb, int tail_ct, bool backward, int workers, bool merged, int nq, const TkOrderOptions& opt)
        : mt(mt), nb(nb), tail_ct(tail_ct), backward(backward), merged(merged), nq(nq < 1 || nq > kMaxQ ? 1 : nq), opt(opt),
          ctiles((nb - 1) * 8 + tail_ct), mt2(mt / 2), ct2(ctiles / 2),
          per_pair((mt2 >= 1 && mt2 <= this->nq && this->nq % mt2 == 0) ? this->nq / mt2 : 1),
          ready_q((size_t)this->nq), free_q((size_t)this->nq, workers / this->nq > 0 ? workers / this->nq : 1),
          up((size_t)mt * ctiles, 0), busy((size_t)mt * ctiles, 0), xs((size_t)mt * nb, 0), xd((size_t)mt * nb, 0), bs((size_t)mt * nb, 0),
          tiles_final((size_t)mt * nb, 0), xready((size_t)mt, 0), bready((size_t)mt, 0) {}

    void run(std::vector<TkItem>& order, std::vector<int>* queues) {
        out = &order;
        queue_of = queues;
        out->clear();
        if (queue_of != nullptr) queue_of->clear();
        for (int r = 0; r < mt; ++r) push_block_items(IT_SB, r, blk_at(0));
        for (;;) {
            for (int q = 0; q < nq; ++q)
                while (free_q[(size_t)q] > 0 && !ready_q[(size_t)q].empty()) {
                    const Ready it = ready_q[(size_t)q].top();
                    ready_q[(size_t)q].pop();
                    start(it, q);
                }
            if (running.empty()) break;
            const Done d = running.top();
            running.pop();
            finish(d);
        }
    }

private:
    const int mt, nb, tail_ct;
    const bool backward, merged;
    const int nq;
    const TkOrderOptions opt;
    const int ctiles;
    const int mt2, ct2;    // 2 x 2 groups: row tiles (2 r2, 2 r2 + 1), column tiles (2 c2, 2 c2 + 1) -- same block (8 | 2 c2)
    const int per_pair;    // pools per pair of row tiles
    std::vector<std::priority_queue<Ready>> ready_q;  // one per pool
    std::vector<int> free_q;                          // idle workers of each pool
    std::priority_queue<Done> running;
    double now = 0.0;
    std::vector<int> up;            // block columns applied to a tile (positions in solve order)
    std::vector<char> busy;         // an update of the tile is queued or running
    std::vector<int> xs, xd, bs, tiles_final;
    std::vector<int> xready;        // positions [0, xready[r]) have their split X
    std::vector<int> bready;        // positions [0, bready[r]) have their split B (the merged chain update's operand)
    std::vector<TkItem>* out = nullptr;
    std::vector<int>* queue_of = nullptr;

    int ct_of(int J) const { return J == nb - 1 ? tail_ct : 8; }
    int pos_of(int J) const { return backward ? nb - 1 - J : J; }  // position of block column J in solve order (0 = solved first)
    int blk_at(int pos) const { return backward ? nb - 1 - pos : pos; }
    size_t tile_id(int r, int c) const { return (size_t)r * ctiles + c; }
    bool paired(int r, int c) const {
        return !opt.no_big && r < 2 * mt2 && c < 2 * ct2 && (c / 8 != nb - 1 || (c % 8) + (c % 2 == 0 ? 1 : 0) < ct_of(nb - 1));
    }
    // an update whose earliest block column (position p0) is the tail-width one of a backward solve: that column goes alone ...
    bool lone_tail(int p0) const { return backward && tail_ct != 8 && p0 == 0; }
    // ... and has tail_ct * 4 k-blocks per block column instead of 32
    int kblocks(int p0) const { return lone_tail(p0) ? tail_ct * 4 : 32; }
    int pool_of(int type, int r, int c) const {  // r: row tile (IT_UB: first of the pair), c: column tile (split items: anything)
        if (nq == 1) return 0;
        const int rp = r / 2;
        if (rp >= mt2) return r % nq;  // the unpaired last row tile
        const int base = (rp * per_pair) % nq;
        if (type == IT_UB) return base + (c / 2) % per_pair;
        return base + (r % 2) % per_pair;  // a row tile's chain (splits, diagonal products, 128 x 128 updates)
    }
    void push(const Ready& it) { ready_q[(size_t)pool_of(it.type, it.r, it.c)].push(it); }

    // the chain update of a tile: only its last block column is missing and that one is split
    void queue_final(int r, int c) {
        const size_t id = tile_id(r, c);
        const int pc = pos_of(c / 8);
        if (busy[id] || pc == 0 || up[id] != pc - 1 || (merged ? bready[r] : xready[r]) < pc) return;
        busy[id] = 1;
        push(Ready{2 * pc - 1, c, r, merged ? IT_UW : IT_U, 0});
    }
    // the update before that (two block columns back): a 128 x 128 item as well -- as part of a 256 x 256 item (~100 us) it would sit
    // between X_J and the chain update of the block after next, i.e. on the chain
    void queue_near(int r, int c) {
        const size_t id = tile_id(r, c);
        const int pc = pos_of(c / 8);
        if (busy[id] || pc < 2 || up[id] != pc - 2 || xready[r] < pc - 1) return;
        busy[id] = 1;
        push(Ready{2 * pc - 1, c, r, IT_U, 0});
    }
    // an unpaired tile takes everything as 128 x 128 items
    void queue_single(int r, int c) {
        const size_t id = tile_id(r, c);
        const int pc = pos_of(c / 8);
        if (busy[id] || up[id] >= pc || up[id] >= xready[r]) return;
        busy[id] = 1;
        push(Ready{2 * pc - 1, c, r, IT_U, 0});
    }
    void queue_pair(int r2, int c2) {
        const int r = 2 * r2, c = 2 * c2;
        const int pc = pos_of(c / 8);
        const int p0 = up[tile_id(r, c)];
        for (int dr = 0; dr < 2; ++dr)
            for (int dc = 0; dc < 2; ++dc)
                if (busy[tile_id(r + dr, c + dc)] || up[tile_id(r + dr, c + dc)] != p0) return;
        const int xr = std::min(xready[r], xready[r + 1]);
        if (std::min(pc - 2, xr) - p0 < 1) return;
        for (int dr = 0; dr < 2; ++dr)
            for (int dc = 0; dc < 2; ++dc) busy[tile_id(r + dr, c + dc)] = 1;
        push(Ready{2 * pc - 1, c, r, IT_UB, 0});
    }
    void requeue_tile(int r, int c) {
        if (paired(r, c)) {
            queue_pair(r / 2, c / 2);
            queue_near(r, c);
            queue_final(r, c);
        } else {
            queue_single(r, c);
        }
    }
    void push_block_items(int type, int r, int J) {
        const int n = type == IT_D ? ct_of(J) : kQ;
        for (int i = 0; i < n; ++i) push(Ready{2 * pos_of(J), type == IT_D ? J * 8 + i : i, r, type, J});
    }

    // a worker of pool q takes the item: its table entry (how many block columns an update takes is decided here) and its finish time
    void start(const Ready& it, int q) {
        TkItem rec;
        Done d{};
        if (it.type == IT_UB) {
            const int r = it.r, c = it.c, pc = pos_of(c / 8);
            const int p0 = up[tile_id(r, c)];
            int avail = std::min(pc - 2, std::min(xready[r], xready[r + 1])) - p0;
            if (avail > opt.max_pan) avail = opt.max_pan;
            if (lone_tail(p0)) avail = 1;
            const int plast = p0 + avail - 1;  // latest block column of the item in solve order = first processed
            rec = TkItem{IT_UB | (avail << 4), r / 2, c / 2, blk_at(plast)};
            d = Done{now + kCost.big0 + kCost.bigstage * kblocks(p0) * avail, IT_UB, r, c, 0, avail};
        } else if (it.type == IT_UW) {
            const int pc = pos_of(it.c / 8);
            const int Jsrc = blk_at(pc - 1);
            rec = TkItem{IT_UW | (1 << 4), it.r, it.c, Jsrc};
            d = Done{now + kCost.tile0 + kCost.stage * 4 * ct_of(Jsrc), IT_UW, it.r, it.c, 0, 1};
        } else if (it.type == IT_U) {
            const int pc = pos_of(it.c / 8);
            const int p0 = up[tile_id(it.r, it.c)];
            int avail = std::min(pc, xready[it.r]) - p0;
            if (avail > opt.max_pan) avail = opt.max_pan;
            if (lone_tail(p0)) avail = 1;
            if (paired(it.r, it.c)) avail = 1;  // the near or the chain update of a paired tile: one block column
            const int plast = p0 + avail - 1;
            rec = TkItem{IT_U | (avail << 4), it.r, it.c, blk_at(plast)};
            d = Done{now + kCost.tile0 + kCost.stage * kblocks(p0) * avail, IT_U, it.r, it.c, 0, avail};
        } else {
            rec = TkItem{it.type | (1 << 4), it.r, it.c, it.J};
            double dur = kCost.split;
            if (it.type == IT_D) {
                const int cl = it.c - it.J * 8;
                const int nk = backward ? (ct_of(it.J) - cl) * 4 : (cl + 1) * 4;
                dur = kCost.tile0 + kCost.stage * nk;
            }
            d = Done{now + dur, it.type, it.r, it.c, it.J, 1};
        }
        out->push_back(rec);
        if (queue_of != nullptr) queue_of->push_back(q);
        d.q = q;
        running.push(d);
        --free_q[(size_t)q];
    }

    // the simulation's clock moves to the item's end: its worker is free, and what it completes is queued
    void finish(const Done& d) {
        now = d.t;
        ++free_q[(size_t)d.q];
        const int r = d.r;
        if (d.type == IT_SB) {
            if (++bs[(size_t)r * nb + d.J] == kQ) {
                push_block_items(IT_D, r, d.J);
                bready[r] = pos_of(d.J) + 1;
                if (merged && pos_of(d.J) + 1 < nb) {
                    const int Jn = blk_at(pos_of(d.J) + 1);
                    for (int c = Jn * 8; c < Jn * 8 + ct_of(Jn); ++c)
                        if (paired(r, c)) queue_final(r, c);
                }
            }
        } else if (d.type == IT_D) {
            if (++xd[(size_t)r * nb + d.J] == ct_of(d.J)) push_block_items(IT_SX, r, d.J);
        } else if (d.type == IT_SX) {
            if (++xs[(size_t)r * nb + d.J] == kQ) {
                xready[r] = pos_of(d.J) + 1;
                for (int c = 0; c < ctiles; ++c)
                    if (pos_of(c / 8) > pos_of(d.J)) requeue_tile(r, c);
            }
        } else {
            const int nr = d.type == IT_UB ? 2 : 1;
            for (int dr = 0; dr < nr; ++dr)
                for (int dc = 0; dc < nr; ++dc) {
                    const size_t id = tile_id(r + dr, d.cq + dc);
                    up[id] += d.npan;
                    busy[id] = 0;
                }
            for (int dr = 0; dr < nr; ++dr)
                for (int dc = 0; dc < nr; ++dc) {
                    const int rr = r + dr, cc = d.cq + dc, Jt = cc / 8;
                    if (up[tile_id(rr, cc)] == pos_of(Jt)) {
                        if (++tiles_final[(size_t)rr * nb + Jt] == ct_of(Jt)) push_block_items(IT_SB, rr, Jt);
                    } else {
                        requeue_tile(rr, cc);
                    }
                }
        }
    }
};

}  // namespace

void tk_build_order(int mt, int nb, int tail_ct, bool backward, int workers, bool merged, std::vector<TkItem>& out, int nq, std::vector<int>* queue_of,
                    const TkOrderOptions& opt) {
    ListScheduler(mt, nb, tail_ct, backward, workers, merged, nq, opt).run(out, queue_of);
}

void tk_layout_tables(const std::vector<TkItem>& order, const std::vector<int>& queue_of, int nq, std::vector<TkItem>& tab, int q_off[kMaxQ + 1]) {
    tab.clear();
    tab.reserve(order.size());
    for (int q = 0; q < nq; ++q) {
        q_off[q] = (int)tab.size();
        for (size_t i = 0; i < order.size(); ++i)
            if (queue_of[i] == q) tab.push_back(order[i]);
    }
    for (int q = nq; q <= kMaxQ; ++q) q_off[q] = (int)tab.size();
}

int tk_order_export(int mt, int nb, int tail_ct, int backward, int workers, int merged, int queues, int32_t* out, int32_t* queue_of, int64_t cap,
                    int64_t* count) {
    if (!(mt >= 1 && nb >= 1 && tail_ct >= 1 && tail_ct <= 8 && workers >= 1 && count != nullptr && (queues == 1 || queues == kMaxQ))) {
        set_error("trsm_ticket_order: bad shape");
        return -2;
    }
    std::vector<TkItem> items;
    std::vector<int> qof;
    tk_build_order(mt, nb, tail_ct, backward != 0, workers, merged != 0, items, queues, &qof);
    *count = (int64_t)items.size();
    if (out != nullptr) {
        if ((int64_t)items.size() > cap) {
            set_error("trsm_ticket_order: %lld items, room for %lld", (long long)items.size(), (long long)cap);
            return -2;
        }
        for (size_t i = 0; i < items.size(); ++i) {
            out[4 * i] = items[i].word; out[4 * i + 1] = items[i].r; out[4 * i + 2] = items[i].c; out[4 * i + 3] = items[i].J;
            if (queue_of != nullptr) queue_of[i] = qof[i];
        }
    }
    return 0;
}

}  // namespace nngp
