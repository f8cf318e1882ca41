// The per-call arithmetic of the launch selection (synthesis_amd/csrc/launch_plan.hpp: launch_query + plan_launch) on a CPU. engine.hip's
// launch_engine builds every query through launch_query, so what holds here holds for a match side's plies (syn_match_run_sides):
//   1. the arithmetic a call carries reaches plan_launch: LaunchQuery::f16 follows it, not the engine;
//   2. an f32 engine with an f16x2 call gets the plan an f16x2 engine gets for its own call, and the reverse, at every launch shape the
//      two arithmetics differ in (the free-running kernel at <= 16 trees per CU, the lane f16 units, conv f16);
//   3. a default-initialised query, and a query built with PLAN_ARITH_ENGINE, plan as before.
// Prints "ok <checks>" and returns 0, or the first difference and 1.
#include <cstdio>
#include <initializer_list>

#include "../../synthesis_amd/csrc/launch_plan.hpp"

using namespace syn;

static bool same_plan(const LaunchPlan& a, const LaunchPlan& b) {
    return a.error == b.error && a.shape == b.shape && a.grid == b.grid && a.threads == b.threads && a.mode == b.mode && a.count == b.count &&
           a.prof == b.prof && a.fast == b.fast && a.n == b.n && a.policy == b.policy && a.tile == b.tile && a.slots == b.slots &&
           a.lane_thresh == b.lane_thresh && a.nv == b.nv && a.debug_prio == b.debug_prio && a.debug_stub == b.debug_stub &&
           a.no_cache == b.no_cache && a.path_entries == b.path_entries && a.vw_bytes == b.vw_bytes && a.pool_trees == b.pool_trees;
}

static int checks = 0;
static int failed(const char* what, int net, int slots, int jobs, int family) {
    std::printf("FAIL %s: net %d slots %d jobs %d family %d\n", what, net, slots, jobs, family);
    return 1;
}

int main() {
    const LaunchKnobs knobs;   // nothing set: the selection a library without SYN_DEBUG makes
    const unsigned cap = 7212; // nodes per tree of a max_explores = 800 engine
    // ---- 1. the truth table of the arithmetic a call evaluates
    const struct { bool engine_f16; int arith; bool want; } table[] = {
        {false, PLAN_ARITH_ENGINE, false}, {true, PLAN_ARITH_ENGINE, true}, {false, PLAN_ARITH_F32, false}, {true, PLAN_ARITH_F32, false},
        {false, PLAN_ARITH_F16X2, true},   {true, PLAN_ARITH_F16X2, true},
    };
    for (const auto& t : table) {
        LaunchEngine e;
        e.f16 = t.engine_f16;
        const LaunchQuery q = launch_query(e, t.arith, 1, 1, false, false, 0, 0, 1);
        checks++;
        if (plan_call_f16(t.engine_f16, t.arith) != t.want || q.f16 != t.want) {
            std::printf("FAIL truth table: engine_f16 %d arith %d -> f16 %d, expected %d\n", (int)t.engine_f16, t.arith, (int)q.f16, (int)t.want);
            return 1;
        }
    }
    // ---- 2. and 3. over networks, sizes, job counts and configuration families
    const int slot_list[] = {16, 32, 64, 4096, 4112, 65536, 131072, 196608, 262144};
    bool saw_free = false, saw_lane_f16 = false, saw_conv_f16 = false, saw_row = false;
    for (int net = 0; net < 2; net++)
        for (int slots : slot_list)
            for (int jobs : {1, 17, slots, 2 * slots})
                for (int family : {0, 1})
                    for (int mode : {0, 1}) {
                        LaunchEngine e32, e16;
                        e32.slots = e16.slots = slots;
                        e32.cap = e16.cap = cap;
                        e32.net_kind = e16.net_kind = net;
                        e32.f16 = false;
                        e16.f16 = true;
                        const int fpu = family == 1 ? 0 : 1;   // family 0: Fpu::ParentQ, a deterministic runtime-switched configuration
                        const auto plan = [&](const LaunchEngine& e, int arith) {
                            return plan_launch(launch_query(e, arith, jobs, mode, false, false, fpu, 0, family), knobs);
                        };
                        const LaunchPlan own16 = plan(e16, PLAN_ARITH_ENGINE), own32 = plan(e32, PLAN_ARITH_ENGINE);
                        checks += 4;
                        if (!same_plan(plan(e32, PLAN_ARITH_F16X2), own16)) return failed("f32 engine, f16x2 call", net, slots, jobs, family);
                        if (!same_plan(plan(e16, PLAN_ARITH_F16X2), own16)) return failed("f16x2 engine, f16x2 call", net, slots, jobs, family);
                        if (!same_plan(plan(e16, PLAN_ARITH_F32), own32)) return failed("f16x2 engine, f32 call", net, slots, jobs, family);
                        if (!same_plan(plan(e32, PLAN_ARITH_F32), own32)) return failed("f32 engine, f32 call", net, slots, jobs, family);
                        // a query filled in by hand, as before the per-call arithmetic existed, plans as the engine's own call does
                        LaunchQuery q;
                        q.slots = slots; q.jobs = jobs; q.cap = cap; q.net_kind = net; q.mode = mode; q.fpu = fpu; q.family = family;
                        checks += 2;
                        if (!same_plan(plan_launch(q, knobs), own32)) return failed("hand-filled f32 query", net, slots, jobs, family);
                        q.f16 = true;
                        if (!same_plan(plan_launch(q, knobs), own16)) return failed("hand-filled f16 query", net, slots, jobs, family);
                        saw_free |= own16.shape == 7;
                        saw_lane_f16 |= own16.shape == 4 && own16.policy == 3;
                        saw_conv_f16 |= own16.shape == 4 && own16.policy == 4;
                        saw_row |= own32.shape == 1 || own32.shape == 2;
                        // the two arithmetics must be told apart somewhere, or the checks above compare a plan with itself
                        if (own16.shape == own32.shape && own16.policy == own32.policy && own16.lane_thresh == own32.lane_thresh && !own16.error)
                            return failed("the f16x2 plan equals the f32 plan", net, slots, jobs, family);
                    }
    if (!saw_free || !saw_lane_f16 || !saw_conv_f16 || !saw_row) {
        std::printf("FAIL coverage: free %d lane-f16 %d conv-f16 %d row %d\n", (int)saw_free, (int)saw_lane_f16, (int)saw_conv_f16, (int)saw_row);
        return 1;
    }
    // ---- 3. a default-initialised query still plans as it did: one row-per-tree workgroup
    {
        const LaunchPlan p = plan_launch(LaunchQuery{}, knobs);
        checks++;
        if (p.error || p.shape != 1 || p.grid != 1 || p.threads != 256 || p.policy != 0 || p.fast != 0) {
            std::printf("FAIL default query: shape %d grid %d threads %d policy %d fast %d\n", p.shape, p.grid, p.threads, p.policy, p.fast);
            return 1;
        }
    }
    std::printf("ok %d\n", checks);
    return 0;
}
