// Stand-alone driver of csrc/trsm_order.cpp for tests/test_trsm_order_host.py: built with the address and undefined-behaviour
// sanitizers, their runtimes linked in, and run as a program of its own (the test preloads nothing and leaves the environment alone).
//   trsm_order_main CASES OUT
// CASES: one case per line, "mt nb tail workers backward merged queues".  OUT receives per case, as int32:
//   mt nb tail workers backward merged queues count | q_off[0..8] | count x {word r c J} | count x queue_of | count x {word r c J}
// i.e. the global start order with each item's queue, then the queue-major device table of tk_layout_tables.
#include <stdarg.h>
#include <stdio.h>

#include <vector>

#include "../../nngp-src_amd/csrc/trsm_order.h"

namespace nngp {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace nngp

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "r");
    FILE* out = fopen(argv[2], "wb");
    if (in == nullptr || out == nullptr) return 2;
    int32_t h[8];
    int cases = 0;
    while (fscanf(in, "%d %d %d %d %d %d %d", &h[0], &h[1], &h[2], &h[3], &h[4], &h[5], &h[6]) == 7) {
        int64_t count = 0;
        if (nngp::tk_order_export(h[0], h[1], h[2], h[4], h[3], h[5], h[6], nullptr, nullptr, 0, &count) != 0) return 1;
        std::vector<nngp::TkItem> order((size_t)count), tab;
        std::vector<int32_t> qof((size_t)count);
        if (nngp::tk_order_export(h[0], h[1], h[2], h[4], h[3], h[5], h[6], reinterpret_cast<int32_t*>(order.data()), qof.data(), count, &count) != 0) return 1;
        int32_t q_off[nngp::kMaxQ + 1];
        nngp::tk_layout_tables(order, std::vector<int>(qof.begin(), qof.end()), h[6], tab, q_off);
        if (tab.size() != order.size()) return 1;
        h[7] = (int32_t)count;
        bool ok = fwrite(h, sizeof(h), 1, out) == 1 && fwrite(q_off, sizeof(q_off), 1, out) == 1;
        if (count > 0)
            ok = ok && fwrite(order.data(), sizeof(nngp::TkItem), order.size(), out) == order.size() &&
                 fwrite(qof.data(), sizeof(int32_t), qof.size(), out) == qof.size() && fwrite(tab.data(), sizeof(nngp::TkItem), tab.size(), out) == tab.size();
        if (!ok) return 2;
        ++cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%d cases\n", cases);
    return 0;
}
