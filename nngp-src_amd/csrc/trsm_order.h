// The work tables of the persistent blocked solves (trsm_tickets.hip): which items exist, in which order they are started and
// which queue each belongs to.  Host code only -- no HIP header -- so that it also builds as a plain C++ program (tests/sanitize).
#pragma once
#include <stdint.h>

#include <vector>

namespace nngp {

void set_error(const char* fmt, ...);

struct TkItem { int32_t word, r, c, J; };  // word = type | panels << 4; the kernel reads the table as int4
enum { IT_SB = 0, IT_D = 1, IT_SX = 2, IT_U = 3, IT_UB = 4, IT_UW = 5 };
constexpr int kQ = 4;                    // split items per (r, J): 32 rows each (8 waves x 4 rows)
constexpr int kMaxQ = 8;

// development aids of the timing-knobs build (tk_dev_switches in trsm_tickets.hip); the product runs the defaults
struct TkOrderOptions {
    int max_pan = 4;      // block columns per update item, 1 .. 4
    bool no_big = false;  // 128 x 128 items only
};

// the global start order of a solve's items (every item behind its dependencies) and, with queue_of, each item's queue
void tk_build_order(int mt, int nb, int tail_ct, bool backward, int workers, bool merged, std::vector<TkItem>& out, int nq = 1,
                    std::vector<int>* queue_of = nullptr, const TkOrderOptions& opt = TkOrderOptions());
// the device table: the queues' tables one behind the other, each in the global start order; queue q = tab[q_off[q] .. q_off[q + 1])
void tk_layout_tables(const std::vector<TkItem>& order, const std::vector<int>& queue_of, int nq, std::vector<TkItem>& tab, int q_off[kMaxQ + 1]);
// the ticket table of a shape (default options), four ints per item {type | panels << 4, r, c or q, J}, for the host-side proof that
// every item's dependencies hold lower tickets (tests/test_host.py)
int tk_order_export(int mt, int nb, int tail_ct, int backward, int workers, int merged, int queues, int32_t* out, int32_t* queue_of, int64_t cap,
                    int64_t* count);

}  // namespace nngp
