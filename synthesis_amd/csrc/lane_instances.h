// synthesis_amd — which instantiations of the self-play kernels the library ships, as X-macro lists: the ONE table of what exists. The side
// translation units define them (engine_lanes_fast.hip: the compile-time-folded parity configuration family, engine_lanes_gen.hip: the
// runtime-switched one, ...; separate units only so that `make -j` builds them beside engine.hip); engine.hip declares them `extern
// template` and expands the same lists into the table its launches are looked up in, so launching code cannot name an instantiation that is
// not listed here. Which entry a call takes is decided in launch_plan.hpp; tests/test_launch_plan.py checks that every plan is listed.
//   X(MODE, COUNT, FAST, NW, PROF, POLICY)      FAST: 0 runtime-switched, 1 parity family, 2 the reference's self-play configuration
//                                                (mcts.cuh CfgView; engine_lanes_ref.hip holds the third list)
#pragma once
#define SYN_LANES_FAST_LIST(X)                                                                                   \
    X(MODE_SELFPLAY, false, true, 4, false, 0) X(MODE_SELFPLAY, false, true, 8, false, 0)                        \
    X(MODE_SELFPLAY, false, true, 12, false, 0) X(MODE_SELFPLAY, false, true, 16, false, 0)                      \
    X(MODE_SELFPLAY, false, true, 4, true, 0) X(MODE_SELFPLAY, false, true, 8, true, 0)                          \
    X(MODE_SELFPLAY, false, true, 12, true, 0) X(MODE_SELFPLAY, false, true, 16, true, 0)                        \
    X(MODE_SELFPLAY, true, true, 4, false, 0) X(MODE_SELFPLAY, true, true, 8, false, 0)                          \
    X(MODE_SELFPLAY, true, true, 12, false, 0) X(MODE_SELFPLAY, true, true, 16, false, 0)                        \
    X(MODE_SEARCH, false, true, 4, false, 0) X(MODE_SEARCH, false, true, 8, false, 0)                            \
    X(MODE_SEARCH, false, true, 12, false, 0) X(MODE_SEARCH, false, true, 16, false, 0)
#define SYN_LANES_GEN_LIST(X)                                                                                    \
    X(MODE_SELFPLAY, false, false, 4, false, 0) X(MODE_SELFPLAY, false, false, 8, false, 0)                      \
    X(MODE_SELFPLAY, false, false, 12, false, 0) X(MODE_SELFPLAY, false, false, 16, false, 0)                    \
    X(MODE_SELFPLAY, false, false, 4, true, 0) X(MODE_SELFPLAY, false, false, 8, true, 0)                        \
    X(MODE_SELFPLAY, false, false, 12, true, 0) X(MODE_SELFPLAY, false, false, 16, true, 0)                      \
    X(MODE_SELFPLAY, true, false, 4, false, 0) X(MODE_SELFPLAY, true, false, 8, false, 0)                        \
    X(MODE_SELFPLAY, true, false, 12, false, 0) X(MODE_SELFPLAY, true, false, 16, false, 0)                      \
    X(MODE_SEARCH, false, false, 4, false, 0) X(MODE_SEARCH, false, false, 8, false, 0)                          \
    X(MODE_SEARCH, false, false, 12, false, 0) X(MODE_SEARCH, false, false, 16, false, 0)                        \
    X(MODE_SEARCH, false, false, 8, false, 1)
#define SYN_LANES_REF_LIST(X)                                                                                    \
    X(MODE_SELFPLAY, false, 2, 8, false, 0) X(MODE_SELFPLAY, false, 2, 16, false, 0)                             \
    X(MODE_SELFPLAY, true, 2, 8, false, 0) X(MODE_SELFPLAY, true, 2, 16, false, 0)                               \
    X(MODE_SEARCH, false, 2, 8, false, 0) X(MODE_SEARCH, false, 2, 16, false, 0)                                 \
    X(MODE_SELFPLAY, false, 2, 8, true, 0) X(MODE_SELFPLAY, false, 2, 16, true, 0)                               \
    X(MODE_SELFPLAY, false, 2, 12, false, 0) X(MODE_SELFPLAY, true, 2, 12, false, 0) X(MODE_SEARCH, false, 2, 12, false, 0) \
    X(MODE_SELFPLAY, false, 2, 12, true, 0)
// Connect4Net in the f16x2 arithmetic (POLICY 3, f16x2_tile.cuh): every configuration family at every wave count
// (engine_lanes_f16.hip)
#define SYN_LANES_F16_LIST(X)                                                                                    \
    X(MODE_SELFPLAY, false, true, 4, false, 3) X(MODE_SELFPLAY, false, true, 8, false, 3)                        \
    X(MODE_SELFPLAY, false, true, 12, false, 3) X(MODE_SELFPLAY, false, true, 16, false, 3)                      \
    X(MODE_SELFPLAY, true, true, 4, false, 3) X(MODE_SELFPLAY, true, true, 8, false, 3)                          \
    X(MODE_SELFPLAY, true, true, 12, false, 3) X(MODE_SELFPLAY, true, true, 16, false, 3)                        \
    X(MODE_SEARCH, false, true, 4, false, 3) X(MODE_SEARCH, false, true, 8, false, 3)                            \
    X(MODE_SEARCH, false, true, 12, false, 3) X(MODE_SEARCH, false, true, 16, false, 3)                          \
    X(MODE_SELFPLAY, false, true, 12, true, 3) X(MODE_SELFPLAY, false, true, 16, true, 3)                        \
    X(MODE_SELFPLAY, false, 2, 4, false, 3) X(MODE_SELFPLAY, false, 2, 8, false, 3)                              \
    X(MODE_SELFPLAY, false, 2, 12, false, 3) X(MODE_SELFPLAY, false, 2, 16, false, 3)                            \
    X(MODE_SELFPLAY, true, 2, 4, false, 3) X(MODE_SELFPLAY, true, 2, 8, false, 3)                                \
    X(MODE_SELFPLAY, true, 2, 12, false, 3) X(MODE_SELFPLAY, true, 2, 16, false, 3)                              \
    X(MODE_SEARCH, false, 2, 4, false, 3) X(MODE_SEARCH, false, 2, 8, false, 3)                                  \
    X(MODE_SEARCH, false, 2, 12, false, 3) X(MODE_SEARCH, false, 2, 16, false, 3)
#define SYN_LANES_F16_GEN_LIST(X)                                                                                \
    X(MODE_SELFPLAY, false, false, 4, false, 3) X(MODE_SELFPLAY, false, false, 8, false, 3)                      \
    X(MODE_SELFPLAY, true, false, 4, false, 3) X(MODE_SELFPLAY, true, false, 8, false, 3)                        \
    X(MODE_SEARCH, false, false, 4, false, 3) X(MODE_SEARCH, false, false, 8, false, 3)
// The pool kernel (pool_kernel.cuh: trees unbound from the lanes for the descent), Connect4Net f32 (POLICY 0: engine_pool.hip) and f16x2
// (POLICY 3: engine_pool_f16.hip), the two compile-time-folded families, 12 waves:  X(MODE, COUNT, FAST, NW, POLICY)
#define SYN_POOL_F32_LIST(X)                                                                                     \
    X(MODE_SELFPLAY, false, 1, 12, 0) X(MODE_SELFPLAY, true, 1, 12, 0) X(MODE_SEARCH, false, 1, 12, 0)           \
    X(MODE_SELFPLAY, false, 2, 12, 0) X(MODE_SELFPLAY, true, 2, 12, 0) X(MODE_SEARCH, false, 2, 12, 0)           \
    X(MODE_SELFPLAY, false, 1, 8, 0) X(MODE_SELFPLAY, true, 1, 8, 0) X(MODE_SEARCH, false, 1, 8, 0)              \
    X(MODE_SELFPLAY, false, 2, 8, 0) X(MODE_SELFPLAY, true, 2, 8, 0) X(MODE_SEARCH, false, 2, 8, 0)
#define SYN_POOL_F16_LIST(X)                                                                                     \
    X(MODE_SELFPLAY, false, 1, 12, 3) X(MODE_SELFPLAY, true, 1, 12, 3) X(MODE_SEARCH, false, 1, 12, 3)           \
    X(MODE_SELFPLAY, false, 2, 12, 3) X(MODE_SELFPLAY, true, 2, 12, 3) X(MODE_SEARCH, false, 2, 12, 3)           \
    X(MODE_SELFPLAY, false, 1, 8, 3) X(MODE_SELFPLAY, true, 1, 8, 3) X(MODE_SEARCH, false, 1, 8, 3)              \
    X(MODE_SELFPLAY, false, 2, 8, 3) X(MODE_SELFPLAY, true, 2, 8, 3) X(MODE_SEARCH, false, 2, 8, 3)
// Connect4ConvNet in the f16x2 arithmetic (POLICY 4, conv_f16x2_tile.cuh; engine_conv_f16.hip): search, self-play and self-play with
// counters, as POLICY 2 ships them, at the wave counts whose instantiations keep their registers: the parity family (FAST true) at 4 and
// 8 waves, the runtime-switched family (FAST false: also the reference's own configuration) at 4
#define SYN_LANES_CONV_F16_LIST(X)                                                                               \
    X(MODE_SEARCH, false, true, 4, false, 4) X(MODE_SEARCH, false, true, 8, false, 4)                            \
    X(MODE_SEARCH, false, false, 4, false, 4)                                                                    \
    X(MODE_SELFPLAY, false, true, 4, false, 4) X(MODE_SELFPLAY, false, true, 8, false, 4)                        \
    X(MODE_SELFPLAY, false, false, 4, false, 4)                                                                  \
    X(MODE_SELFPLAY, true, true, 4, false, 4) X(MODE_SELFPLAY, true, true, 8, false, 4)                          \
    X(MODE_SELFPLAY, true, false, 4, false, 4)
// Connect4ConvNet in f32 (POLICY 2, convnet.cuh; engine_conv.hip): both runtime values of FAST at 4, 8 and 16 waves
#define SYN_LANES_CONV_LIST(X) \
    X(MODE_SEARCH, false, true, 4, false, 2) X(MODE_SEARCH, false, false, 4, false, 2) \
    X(MODE_SEARCH, false, true, 8, false, 2) X(MODE_SEARCH, false, false, 8, false, 2) \
    X(MODE_SEARCH, false, true, 16, false, 2) X(MODE_SEARCH, false, false, 16, false, 2) \
    X(MODE_SELFPLAY, false, true, 4, false, 2) X(MODE_SELFPLAY, false, false, 4, false, 2) \
    X(MODE_SELFPLAY, false, true, 8, false, 2) X(MODE_SELFPLAY, false, false, 8, false, 2) \
    X(MODE_SELFPLAY, false, true, 16, false, 2) X(MODE_SELFPLAY, false, false, 16, false, 2) \
    X(MODE_SELFPLAY, true, true, 4, false, 2) X(MODE_SELFPLAY, true, false, 4, false, 2) \
    X(MODE_SELFPLAY, true, true, 8, false, 2) X(MODE_SELFPLAY, true, false, 8, false, 2) \
    X(MODE_SELFPLAY, true, true, 16, false, 2) X(MODE_SELFPLAY, true, false, 16, false, 2)
// The free-running four-trees-per-wave kernels (free_kernel.cuh; engine_free.hip):  X(MODE, COUNT, FAST, PROF)
#define SYN_FREE_LIST(X) \
    X(MODE_SEARCH, false, true, false) X(MODE_SEARCH, false, false, false) \
    X(MODE_SELFPLAY, false, true, false) X(MODE_SELFPLAY, false, false, false) \
    X(MODE_SELFPLAY, true, true, false) X(MODE_SELFPLAY, true, false, false) \
    X(MODE_SELFPLAY, false, true, true)
// (DEBUG_SHAPES=1 builds) the two-trees-per-lane kernels (lane2_kernel.cuh; engine_lanes2.hip):  X(MODE, COUNT, FAST, NW, POLICY, TILE)
#define SYN_LANES2_LIST(X) \
    X(MODE_SEARCH, false, true, 8, 0, 0) X(MODE_SEARCH, false, false, 8, 0, 0) \
    X(MODE_SEARCH, false, true, 8, 2, 0) X(MODE_SEARCH, false, false, 8, 2, 0) \
    X(MODE_SEARCH, false, true, 12, 0, 0) X(MODE_SEARCH, false, false, 12, 0, 0) \
    X(MODE_SEARCH, false, true, 12, 2, 0) X(MODE_SEARCH, false, false, 12, 2, 0) \
    X(MODE_SELFPLAY, false, true, 8, 0, 0) X(MODE_SELFPLAY, false, false, 8, 0, 0) \
    X(MODE_SELFPLAY, false, true, 8, 2, 0) X(MODE_SELFPLAY, false, false, 8, 2, 0) \
    X(MODE_SELFPLAY, false, true, 12, 0, 0) X(MODE_SELFPLAY, false, false, 12, 0, 0) \
    X(MODE_SELFPLAY, false, true, 12, 2, 0) X(MODE_SELFPLAY, false, false, 12, 2, 0) \
    X(MODE_SELFPLAY, true, true, 8, 0, 0) X(MODE_SELFPLAY, true, false, 8, 0, 0) \
    X(MODE_SELFPLAY, true, true, 8, 2, 0) X(MODE_SELFPLAY, true, false, 8, 2, 0) \
    X(MODE_SELFPLAY, true, true, 12, 0, 0) X(MODE_SELFPLAY, true, false, 12, 0, 0) \
    X(MODE_SELFPLAY, true, true, 12, 2, 0) X(MODE_SELFPLAY, true, false, 12, 2, 0) \
    X(MODE_SELFPLAY, false, true, 8, 0, 1)
