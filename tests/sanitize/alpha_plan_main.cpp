// Stand-alone driver of csrc/alpha_plan.h for tests/test_alpha_plan_host.py: built with the address and undefined-behaviour
// sanitizers, their runtimes linked in, and run as a program of its own (the test preloads nothing and leaves the environment alone).
//   alpha_plan_main SCRIPT
// SCRIPT: one command per line, run in order on ONE record:
//   request MAX_ITERS TOL REG REG_FAC | installed ITERS RELRES | drop | invalidate | begin | note IT RR | stopped IT | event |
//   next ALLOW_PARTIAL | early ALLOW_PARTIAL NY NEVER
// After each command one line goes to stdout: "solved pending partial iters_done max_iters tol iters relres have_event result"
// (result: next -> 0 OrderOnly, 1 Resume, 2 Fresh; early -> 0 / 1; 0 for the others).  `event` stands for the recording of ev_solved.
#include <stdio.h>
#include <string.h>

#include "../../nngp-src_amd/csrc/alpha_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (in == nullptr) return 2;
    nngp::AlphaPlan p;
    char cmd[16];
    int lines = 0;
    while (fscanf(in, "%15s", cmd) == 1) {
        int result = 0, a = 0, b = 0, c = 0;
        double x = 0.0, y = 0.0, z = 0.0;
        if (strcmp(cmd, "request") == 0) {
            if (fscanf(in, "%d %lf %lf %lf", &a, &x, &y, &z) != 4) return 2;
            p.request(a, x, y, z);
        } else if (strcmp(cmd, "installed") == 0) {
            if (fscanf(in, "%d %lf", &a, &x) != 2) return 2;
            p.installed(a, x);
        } else if (strcmp(cmd, "drop") == 0) {
            p.drop();
        } else if (strcmp(cmd, "invalidate") == 0) {
            p.invalidate();
        } else if (strcmp(cmd, "begin") == 0) {
            p.begin_run();
        } else if (strcmp(cmd, "note") == 0) {
            if (fscanf(in, "%d %lf", &a, &x) != 2) return 2;
            p.note(a, x);
        } else if (strcmp(cmd, "stopped") == 0) {
            if (fscanf(in, "%d", &a) != 1) return 2;
            p.stopped_early(a);
        } else if (strcmp(cmd, "event") == 0) {
            p.have_event = true;
        } else if (strcmp(cmd, "next") == 0) {
            if (fscanf(in, "%d", &a) != 1) return 2;
            const nngp::AlphaNext n = p.next(a != 0);
            result = n == nngp::AlphaNext::Fresh ? 2 : n == nngp::AlphaNext::Resume ? 1 : 0;
        } else if (strcmp(cmd, "early") == 0) {
            if (fscanf(in, "%d %d %d", &a, &b, &c) != 3) return 2;
            result = p.may_stop_early(a != 0, b, c != 0) ? 1 : 0;
        } else {
            return 2;
        }
        printf("%d %d %d %d %d %.17g %d %.17g %d %d\n", p.solved ? 1 : 0, p.pending ? 1 : 0, p.partial ? 1 : 0, p.iters_done, p.max_iters,
               p.tol, p.iters, p.relres, p.have_event ? 1 : 0, result);
        ++lines;
    }
    fclose(in);
    return lines > 0 ? 0 : 2;
}
