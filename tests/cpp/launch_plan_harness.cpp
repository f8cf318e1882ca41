// Prints the launch plan (synthesis_amd/csrc/launch_plan.hpp) for queries given on stdin, one per line, as key=value tokens:
//   query fields   cus slots jobs cap net f16 pool_trees mode count prof fpu noise fam   (defaults: LaunchQuery's, cus 256)
//   knobs          SYN_LANES SYN_FREE SYN_QUADS SYN_LANE_THRESH SYN_SCAN_MIN SYN_ABLATE SYN_PC SYN_PC_PRIO SYN_PC_STUB SYN_LANES2 SYN_L2_TILE
//                  SYN_POOL SYN_POOL_NW SYN_POOL_FIRE SYN_POOL_SCAN
//   rollout=1      the RolloutPolicy search's plan for (slots, jobs, cap)
//   eval=1         the policy-evaluation plan (plan_eval) for (net, f16, n, cus, poll_max, zc_out, poll_broken); its output line is
//                  kernel threads grid lds f16_image in_place polled
// Output per line: error shape grid threads fast n policy tile prof slots lane_thresh nv path_entries listed
// listed: 1 = the plan's kernel is in lane_instances.h's lists (or is one of the kernels engine.hip instantiates itself for every call:
// row-per-tree, quads, producer/consumer), 2 = only its unprofiled twin is, 0 = neither.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <sstream>
#include <string>
#include <tuple>

#include "../../synthesis_amd/csrc/lane_instances.h"
#include "../../synthesis_amd/csrc/launch_plan.hpp"

enum { MODE_SELFPLAY = 0, MODE_SEARCH = 1 };
using Key = std::tuple<int, int, int, int, int, int, int, int>;   // shape, mode, count, fast, n, prof, policy, tile

static std::set<Key> shipped() {
    std::set<Key> s;
#define SYN_X(MODE, COUNT, FAST, NW, PROF, POLICY) s.insert(Key{4, MODE, COUNT, FAST, NW, PROF, POLICY, 0});
    SYN_LANES_FAST_LIST(SYN_X) SYN_LANES_GEN_LIST(SYN_X) SYN_LANES_REF_LIST(SYN_X) SYN_LANES_F16_LIST(SYN_X) SYN_LANES_F16_GEN_LIST(SYN_X)
    SYN_LANES_CONV_LIST(SYN_X) SYN_LANES_CONV_F16_LIST(SYN_X)
#undef SYN_X
#define SYN_X(MODE, COUNT, FAST, PROF) s.insert(Key{7, MODE, COUNT, FAST, 0, PROF, 0, 0});
    SYN_FREE_LIST(SYN_X)
#undef SYN_X
#ifdef SYN_DEBUG_SHAPES
#define SYN_X(MODE, COUNT, FAST, NW, POLICY, TILE) s.insert(Key{6, MODE, COUNT, FAST, NW, 0, POLICY, TILE});
    SYN_LANES2_LIST(SYN_X)
#undef SYN_X
#define SYN_X(MODE, COUNT, FAST, NW, POLICY) s.insert(Key{8, MODE, COUNT, FAST, NW, 0, POLICY, 0});
    SYN_POOL_F32_LIST(SYN_X) SYN_POOL_F16_LIST(SYN_X)
#undef SYN_X
#endif
    return s;
}

int main() {
    const std::set<Key> have = shipped();
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        syn::LaunchQuery q;
        syn::LaunchKnobs k;
        int rollout = 0, eval = 0;
        syn::EvalQuery ev;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { std::fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
            const std::string key = tok.substr(0, eq);
            const long long v = std::atoll(tok.c_str() + eq + 1);
            const struct { const char* name; int* p; } ints[] = {
                {"cus", &q.num_cus}, {"slots", &q.slots}, {"jobs", &q.jobs}, {"net", &q.net_kind}, {"pool_trees", &q.pool_trees}, {"mode", &q.mode},
                {"fpu", &q.fpu}, {"noise", &q.noise}, {"fam", &q.family}, {"rollout", &rollout},
                {"eval", &eval}, {"n", &ev.n},
                {"SYN_LANES", &k.lanes}, {"SYN_FREE", &k.free_run}, {"SYN_QUADS", &k.quads}, {"SYN_LANE_THRESH", &k.lane_thresh},
                {"SYN_SCAN_MIN", &k.scan_min}, {"SYN_ABLATE", &k.ablate}, {"SYN_PC", &k.pc}, {"SYN_PC_PRIO", &k.pc_prio}, {"SYN_PC_STUB", &k.pc_stub},
                {"SYN_LANES2", &k.lanes2}, {"SYN_L2_TILE", &k.l2_tile}, {"SYN_POOL", &k.pool}, {"SYN_POOL_NW", &k.pool_nw},
                {"SYN_POOL_FIRE", &k.pool_fire}, {"SYN_POOL_SCAN", &k.pool_scan}};
            bool found = false;
            for (const auto& f : ints)
                if (key == f.name) { *f.p = (int)v; found = true; }
            if (key == "cap") { q.cap = (unsigned)v; found = true; }
            if (key == "f16") { q.f16 = v != 0; found = true; }
            if (key == "count") { q.count = v != 0; found = true; }
            if (key == "prof") { q.prof = v != 0; found = true; }
            if (key == "poll_max") { ev.poll_max = (size_t)v; found = true; }
            if (key == "zc_out") { ev.zero_copy_out = (size_t)v; found = true; }
            if (key == "poll_broken") { ev.poll_broken = v != 0; found = true; }
            if (!found) { std::fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        if (eval) {
            ev.net_kind = q.net_kind; ev.f16 = q.f16; ev.num_cus = q.num_cus;
            const syn::EvalPlan e = syn::plan_eval(ev);
            std::printf("%d %d %d %zu %d %d %d\n", e.kernel, e.threads, e.grid, e.lds, (int)e.f16_image, (int)e.in_place, (int)e.polled);
            continue;
        }
        const syn::LaunchPlan p = rollout ? syn::plan_rollout_search(q.slots, q.jobs, q.cap) : syn::plan_launch(q, k);
        int listed = 0;
        if (!p.error) {
            const Key exact{p.shape, p.mode, p.count, p.fast, p.n, p.prof, p.policy, p.tile};
            Key plain = exact;
            std::get<5>(plain) = 0;
            const bool own = p.shape <= 3 || p.shape == 5;   // instantiated by engine.hip for every kind of call, FAST 0 / 1
            if (own) listed = (p.fast == 0 || p.fast == 1) && (p.shape == 5 || (p.shape == 3 ? p.n >= 2 && p.n <= 4 : p.n == p.shape));
            else listed = have.count(exact) ? 1 : (have.count(plain) ? 2 : 0);
        }
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %zu %d\n", (int)p.error, p.shape, p.grid, p.threads, p.fast, p.n, p.policy, p.tile,
                    (int)p.prof, p.slots, p.lane_thresh, p.nv, p.path_entries, listed);
    }
    return 0;
}
