// Prints the plan of a micro-batch gradient launch (synthesis_amd/csrc/launch_plan.hpp: plan_micro_grads) for queries given on stdin,
// one per line, as key=value tokens: net nb cap cus (defaults: MicroQuery's).
// Output per line: grid threads lds row_stride buffer_bytes reduce_grid reduce_threads
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

#include "../../synthesis_amd/csrc/launch_plan.hpp"

int main() {
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        syn::MicroQuery q;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { std::fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
            const std::string key = tok.substr(0, eq);
            const int v = std::atoi(tok.c_str() + eq + 1);
            if (key == "net") q.net_kind = v;
            else if (key == "nb") q.nb = v;
            else if (key == "cap") q.max_workgroups = v;
            else if (key == "cus") q.num_cus = v;
            else { std::fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        const syn::MicroPlan p = syn::plan_micro_grads(q);
        std::printf("%d %d %zu %d %zu %d %d\n", p.grid, p.threads, p.lds, p.row_stride, p.buffer_bytes, p.reduce_grid, p.reduce_threads);
    }
    return 0;
}
