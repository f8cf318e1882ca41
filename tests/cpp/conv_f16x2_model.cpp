// TEST INFRASTRUCTURE ONLY — the CPU restatement of Connect4ConvNet in the f16x2 arithmetic (the definition at the top of
// synthesis_amd/csrc/conv_f16x2_tile.cuh), bit for bit, on the oracle's model of v_mfma_f32_16x16x32_f16 (oracle/nn_f16x2.hpp
// mfma_f16_k32, unchanged), plus the oracle's own search and self-play drivers instantiated with it. Built by tests/conv_f16x2_model.py
// with the oracle's compiler flags (oracle/Makefile): other flags can change the f32 rounding.
//
// Exports (argument layouts of the oracle's orc_c4conv_* calls, tests/oracle_lib.py):
//   cf16_num_params, cf16_eval, cf16_plan, cf16_mcts_search, cf16_selfplay
#include "../../oracle/oracle_capi.cpp"

namespace cf16model {
using namespace oracle;

struct Plan {
    bool ok = false;
    int tc = 0, s1 = 0, th = 0, out_exp = 0;
    double bound[2] = {0, 0};
    F16Dec cw_hi[16][32], cw_lo[16][32];          // conv weights of channel ch, k = tap (taps 18..31 zero)
    std::vector<F16Dec> hw_hi, hw_lo;             // head weights [o 12][kb 32][k 32]
    float cbias[16], hbias[12];                   // b 2^tc, b 2^(s1 + th)
    float cs = 1.0f, os = 1.0f;                   // 2^(s1 - tc), 2^-(s1 + th)
};

static int weight_exp(const float* w, size_t n, bool& ok) {
    double m = 0;
    for (size_t i = 0; i < n; i++) {
        if (!std::isfinite(w[i])) ok = false;
        m = std::fmax(m, std::fabs((double)w[i]));
    }
    const int t = m > 0 ? 14 - ceil_log2_pos(m) : 0;
    return t > 40 ? 40 : t;
}
static void split(float w, int e, uint16_t& hi, uint16_t& lo) {
    const float ws = std::ldexp(w, e);
    hi = f16_bits_rne(ws);
    lo = f16_bits_rne(ws - f16_value(hi));
}

static void make_plan(const float* blob, Plan& P) {
    using N = Connect4ConvNet;
    const float* cw = blob;
    const float* cb = blob + N::CONV_W;
    const float* hw = cb + N::C;
    const float* hb = hw + (size_t)N::OUT * N::FLAT;
    bool ok = true;
    P.tc = weight_exp(cw, N::CONV_W, ok);
    P.th = weight_exp(hw, (size_t)N::OUT * N::FLAT, ok);
    for (int i = 0; i < N::C; i++) ok = ok && std::isfinite(cb[i]);
    for (int i = 0; i < N::OUT; i++) ok = ok && std::isfinite(hb[i]);
    P.ok = false;
    if (!ok) return;
    // the conv pre-activation of channel ch is at most b + the sum of its positive tap weights (inputs 0 / 1); the head's inputs are
    // bounded by their channel's bound
    double ub[16], B0 = 0, B1 = 0;
    for (int ch = 0; ch < 16; ch++) {
        double a = (double)cb[ch];
        for (int t = 0; t < 18; t++) a += std::fmax((double)cw[ch * 18 + t], 0.0);
        ub[ch] = a > 0 ? a : 0.0;
        B0 = std::fmax(B0, ub[ch]);
    }
    for (int o = 0; o < N::OUT; o++) {
        double a = (double)hb[o];
        for (int i = 0; i < N::FLAT; i++) a += std::fmax((double)hw[(size_t)o * N::FLAT + i], 0.0) * ub[i / N::HW];
        B1 = std::fmax(B1, std::fabs(a));
    }
    P.bound[0] = B0;
    P.bound[1] = B1;
    P.s1 = 15 - ceil_log2_pos(std::fmax(B0, 1e-30));
    if (P.s1 > 24) P.s1 = 24;
    const int eh = P.s1 + P.th;
    if (P.tc < -60 || P.tc > 60 || eh < -60 || eh > 60) return;
    P.out_exp = -eh;
    for (int i = 0; i < 16; i++) {
        P.cbias[i] = std::ldexp(cb[i], P.tc);
        if (!std::isfinite(P.cbias[i])) return;
    }
    for (int o = 0; o < N::OUT; o++) {
        P.hbias[o] = std::ldexp(hb[o], eh);
        if (!std::isfinite(P.hbias[o])) return;
    }
    for (int ch = 0; ch < 16; ch++)
        for (int k = 0; k < 32; k++) {
            uint16_t hi = 0, lo = 0;
            if (k < 18) split(cw[ch * 18 + k], P.tc, hi, lo);
            P.cw_hi[ch][k] = f16_dec(hi);
            P.cw_lo[ch][k] = f16_dec(lo);
        }
    P.hw_hi.assign((size_t)N::OUT * 32 * 32, F16Dec{0, 0});
    P.hw_lo.assign((size_t)N::OUT * 32 * 32, F16Dec{0, 0});
    for (int o = 0; o < N::OUT; o++)
        for (int kb = 0; kb < 32; kb++)
            for (int k = 0; k < 32; k++) {
                const int q = k >> 3, jj = k & 7, ch = 4 * q + (jj & 3), b = 2 * kb + (jj >> 2);
                if (b >= 63) continue;   // bit 63: no cell
                uint16_t hi, lo;
                split(hw[(size_t)o * N::FLAT + ch * N::HW + (b % 7) * 9 + b / 7], P.th, hi, lo);
                P.hw_hi[((size_t)o * 32 + kb) * 32 + k] = f16_dec(hi);
                P.hw_lo[((size_t)o * 32 + kb) * 32 + k] = f16_dec(lo);
            }
    P.cs = std::ldexp(1.0f, P.s1 - P.tc);
    P.os = std::ldexp(1.0f, P.out_exp);
    P.ok = true;
}

// the 12 raw outputs of one position
static void forward(const Plan& P, uint64_t my, uint64_t op, float* out12) {
    // conv: every board bit b = row + 7 col (b = 63: no cell, all inputs 0), taps t = ci*9 + k1*3 + k2 in the instruction's k order
    static const uint16_t ONE = 0x3C00;
    uint16_t ah[64][16], al[64][16];
    for (int b = 0; b < 64; b++) {
        F16Dec x[32];
        for (int t = 0; t < 32; t++) {
            bool on = false;
            if (t < 18 && b < 63) {
                const int ci = t / 9, k1 = (t % 9) / 3, k2 = t % 3;
                const int r = b % 7 + k1 - 1, c = b / 7 + k2 - 1;
                if (r >= 0 && r < 7 && c >= 0 && c < 9) on = (((ci ? op : my) >> (r + 7 * c)) & 1ull) != 0;
            }
            x[t] = f16_dec(on ? ONE : 0);
        }
        for (int ch = 0; ch < 16; ch++) {
            float acc = P.cbias[ch];
            acc = mfma_f16_k32_dec(acc, P.cw_hi[ch], x);
            acc = mfma_f16_k32_dec(acc, P.cw_lo[ch], x);
            float a = acc * P.cs;
            a = (a != a) ? 0.0f : (a < 0.0f ? 0.0f : (a > 65504.0f ? 65504.0f : a));
            ah[b][ch] = f16_bits_rne(a);
            al[b][ch] = f16_bits_rne(a - f16_value(ah[b][ch]));
        }
    }
    // head: block kb = board bits 2kb, 2kb + 1 x 16 channels, k = 8 q + jj -> channel 4q + (jj & 3) of bit 2kb + (jj >> 2)
    for (int o = 0; o < 12; o++) out12[o] = P.hbias[o];
    for (int kb = 0; kb < 32; kb++) {
        F16Dec xh[32], xl[32];
        for (int k = 0; k < 32; k++) {
            const int q = k >> 3, jj = k & 7, ch = 4 * q + (jj & 3), b = 2 * kb + (jj >> 2);
            xh[k] = f16_dec(ah[b][ch]);
            xl[k] = f16_dec(al[b][ch]);
        }
        for (int o = 0; o < 12; o++) {
            const F16Dec* wh = &P.hw_hi[((size_t)o * 32 + kb) * 32];
            const F16Dec* wl = &P.hw_lo[((size_t)o * 32 + kb) * 32];
            float c = out12[o];
            c = mfma_f16_k32_dec(c, wh, xh);
            c = mfma_f16_k32_dec(c, wh, xl);
            c = mfma_f16_k32_dec(c, wl, xh);
            out12[o] = c;
        }
    }
    for (int o = 0; o < 12; o++) out12[o] = out12[o] * P.os;
}

// The interface the oracle's drivers use (oracle/nn.hpp Connect4Net / Connect4ConvNet): blob, mode, eval. The plan is built from the
// blob on first use (one object per worker thread).
struct ConvF16x2Net {
    static constexpr size_t NUM_PARAMS = Connect4ConvNet::NUM_PARAMS;
    const float* blob = nullptr;
    int mode = ACC_F16X2;
    mutable std::shared_ptr<Plan> plan;
    mutable const float* plan_blob = nullptr;
    const Plan& get() const {
        if (!plan || plan_blob != blob) {
            plan = std::make_shared<Plan>();
            make_plan(blob, *plan);
            plan_blob = blob;
        }
        return *plan;
    }
    void eval(const Connect4& game, float logits[9], float value[3]) const {
        float out[12];
        forward(get(), game.my_bb, game.op_bb, out);
        for (int i = 0; i < 9; i++) logits[i] = out[i];
        softmax_stable(out + 9, value, 3);
    }
};

}  // namespace cf16model

using cf16model::ConvF16x2Net;

extern "C" {

size_t cf16_num_params() { return ConvF16x2Net::NUM_PARAMS; }

// logits[n][9], value[n][3], raw12 (optional) [n][12]; mode is ignored (always the f16x2 arithmetic)
void cf16_eval(const float* blob, const uint64_t* my_bb, const uint64_t* op_bb, int n, float* logits, float* value, float* raw12,
               int mode) {
    (void)mode;
    ConvF16x2Net net;
    net.blob = blob;
    const cf16model::Plan& P = net.get();
    for (int i = 0; i < n; i++) {
        float out[12];
        cf16model::forward(P, my_bb[i], op_bb[i], out);
        for (int k = 0; k < 9; k++) logits[(size_t)i * 9 + k] = out[k];
        softmax_stable(out + 9, value + (size_t)i * 3, 3);
        if (raw12)
            for (int k = 0; k < 12; k++) raw12[(size_t)i * 12 + k] = out[k];
    }
}

// exps = {tc, s1, th, out_exp}, bound = {conv activations, head outputs}; returns 1 when the blob has a plan
int cf16_plan(const float* blob, int* exps, double* bound) {
    cf16model::Plan P;
    cf16model::make_plan(blob, P);
    exps[0] = P.tc; exps[1] = P.s1; exps[2] = P.th; exps[3] = P.out_exp;
    bound[0] = P.bound[0]; bound[1] = P.bound[1];
    return P.ok ? 1 : 0;
}

void cf16_mcts_search(const orc_mcts_config* cfg_in, const float* blob, int nn_mode, const uint64_t* my_bb, const uint64_t* op_bb, int n,
                      int explores, int action_selection, float* child_N, float* child_W, float* child_P, int* child_sol,
                      float* root_stat, int* root_sol, unsigned* num_nodes, int* best_action, float* target_pi, float* target_q) {
    c4_mcts_search_impl<ConvF16x2Net>(cfg_in, blob, nn_mode, my_bb, op_bb, n, explores, action_selection, child_N, child_W, child_P,
                                      child_sol, root_stat, root_sol, num_nodes, best_action, target_pi, target_q);
}

double cf16_selfplay(const orc_rollout_config* cfg_in, const float* blob, int nn_mode, uint64_t base_seed, uint64_t first_game,
                     int n_games, int threads, int use_cache, int* plies, uint64_t* states_bb, float* pis, float* vs, uint8_t* actions,
                     uint32_t* root_nodes, uint8_t* final_kind, uint64_t* counters) {
    return c4_selfplay_impl<ConvF16x2Net>(cfg_in, blob, nn_mode, base_seed, first_game, n_games, threads, use_cache, plies, states_bb,
                                          pis, vs, actions, root_nodes, final_kind, counters);
}

}  // extern "C"
