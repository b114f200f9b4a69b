// Stand-alone driver of csrc/i8_trust.h for tests/test_i8_trust_host.py: built with the address and undefined-behaviour sanitizers,
// their runtimes linked in, and run as a program of its own (the test preloads nothing and leaves the environment alone).
//   i8_trust_main SCRIPT
// SCRIPT: one command per line, run in order on ONE trust record:
//   new | pending | first RATIO THRESHOLD | fold RATIO THRESHOLD | coarse NP MP | fine NP MP
// After each command one line goes to stdout: "checked distrusted pending floor_ratio result" (result: what first / coarse / fine
// returned, 0 for the others).
#include <stdio.h>
#include <string.h>

#include "../../nngp-src_amd/csrc/i8_trust.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (in == nullptr) return 2;
    nngp::I8Trust t;
    char cmd[16];
    int lines = 0;
    while (fscanf(in, "%15s", cmd) == 1) {
        int result = 0;
        double ratio = 0.0, thr = 0.0;
        long long np = 0, mp = 0;
        if (strcmp(cmd, "new") == 0) {
            t.new_kernel();
        } else if (strcmp(cmd, "pending") == 0) {
            t.pending = true;
        } else if (strcmp(cmd, "first") == 0 || strcmp(cmd, "fold") == 0) {
            if (fscanf(in, "%lf %lf", &ratio, &thr) != 2) return 2;
            if (cmd[1] == 'i') result = t.first_verdict(ratio, thr) ? 1 : 0;
            else t.fold(ratio, thr);
        } else if (strcmp(cmd, "coarse") == 0 || strcmp(cmd, "fine") == 0) {
            if (fscanf(in, "%lld %lld", &np, &mp) != 2) return 2;
            result = (cmd[0] == 'c' ? nngp::i8_coarse_pays(np, mp) : nngp::i8_fine_pays(np, mp)) ? 1 : 0;
        } else {
            return 2;
        }
        printf("%d %d %d %.17g %d\n", t.checked ? 1 : 0, t.distrusted ? 1 : 0, t.pending ? 1 : 0, t.floor_ratio, result);
        ++lines;
    }
    fclose(in);
    return lines > 0 ? 0 : 2;
}
