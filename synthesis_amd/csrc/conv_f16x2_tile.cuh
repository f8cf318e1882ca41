// synthesis_amd — Connect4ConvNet leaf evaluation in the f16x2 arithmetic: the network of convnet.cuh (Conv2d<2, 16, 3, pad 1> +
// ReLU + Linear<1008, 12>, oracle/nn.hpp Connect4ConvNet) with every weight and activation as a pair of f16 numbers on
// v_mfma_f32_16x16x32_f16, the split of f16x2_tile.cuh carried over to the conv layer.
//
// Definition (every scale an exact power of two, chosen per checkpoint at load time by build_conv_f16x2_image):
//   plan      tc = 14 - ceil_log2(max |Wc|)  (0 when all conv weights are zero, at most 40);
//             bound_ch = b_ch + sum over the 18 taps (ci -> k1 -> k2) of max(w, 0)   (f64, taps ascending; the inputs are 0 / 1,
//             so this is the exact maximum of channel ch's pre-activation over interior cells);  ub_ch = max(bound_ch, 0);
//             bound[0] = max_ch ub_ch;  s1 = min(24, 15 - ceil_log2(max(bound[0], 1e-30)));
//             th = 14 - ceil_log2(max |Wh|) (0 / at most 40 as above);  bound[1] = max_o |b_o + sum_i max(w_oi, 0) ub_{ch(i)}|
//             (f64, i = ch*63 + row*9 + col ascending);  no plan when a parameter is not finite or tc, s1 + th leave [-60, 60].
//   conv      operands  w' = w 2^tc:  w_hi = RNE_f16(w'), w_lo = RNE_f16(w' - w_hi);  inputs x = the 0 / 1 bitplanes (f16 1.0 = 0x3C00:
//             exact, no scale).  For every board cell, acc_ch = b_ch 2^tc;  acc = M(acc, w_hi, x);  acc = M(acc, w_lo, x)  — k = tap
//             t = ci*9 + k1*3 + k2 (slimnn's order), taps 18..31 zero weights against zero inputs; a tap in the padding reads 0.
//             The products w.x are exact: nothing is dropped but what M's own alignment drops.
//   ReLU      a = med3(acc 2^(s1 - tc), 0, 65504) (NaN -> 0), a_hi = RNE_f16(a), a_lo = RNE_f16(a - a_hi).
//   head      w' = w 2^th split as above;  acc_o = b_o 2^(s1 + th);  per block kb = 0..31 of 32 inputs:  acc = M(acc, w_hi, a_hi);
//             acc = M(acc, w_hi, a_lo);  acc = M(acc, w_lo, a_hi).  Input k = 8 q + jj of block kb = channel 4 q + (jj & 3) of board
//             bit b = 2 kb + (jj >> 2) (bit b = row + 7 col, connect4.rs:108-114) = flat input (4 q + (jj & 3)) * 63 + (b % 7) * 9 + b / 7;
//             bit 63 is no cell: its inputs carry zero weights (1,008 inputs = 31.5 blocks).
//   outputs   raw_o = acc_o 2^-(s1 + th) (one f32 multiply); logits = raw[0..9], value = softmax(raw[9..12]) as oracle/nn.hpp.
//   M(c,a,b)  one v_mfma_f32_16x16x32_f16 (oracle/nn_f16x2.hpp mfma_f16_k32: four passes of eight k, k = 8 q + jj).
// tests/cpp/conv_f16x2_model.cpp restates this on the CPU bit for bit. Like Connect4Net's f16x2 it is a definition of its own, not
// bit-identical to the f32 path (convnet.cuh / ACC_FMA); the two agree to f32 rounding noise.
//
// Fragment layout (lane l: i = l & 15, q = l >> 4; A[i][8q + jj], B[8q + jj][j = i], D[4q + r][j]):
//   conv  A = conv weights (row i = channel, k = tap): two registers-quads per lane for the whole tile (hi, lo); B = the tap bits of
//         position j; D = channels 4q..4q+3 of position j at that cell.
//   head  A = head weights (row i = output o, 12..15 zero); B = activations: slot jj < 4 = the D register jj of the even cell 2kb,
//         jj >= 4 = D register jj - 4 of the odd cell 2kb + 1 — the conv tile's D registers ARE the head's B operands, no cross-lane
//         movement (the trick f16x2_tile.cuh uses between MLP layers); the head-weight image is permuted to match.
// Per tile of 16 positions: 63 x 2 conv + 32 x 3 head = 222 MFMAs (16 matrix cycles each: 3.6k cycles; the f32 tile: 567 x 32).
// Measured (profiles/r07_conv_arith_ab.json): self-play at the bench's conv shape 103.6k games/s against 62.7k in f32.
#pragma once
#include "convnet.cuh"
#include "f16x2_tile.cuh"

namespace syn {

struct ConvF16Geom {
    static constexpr int NKB = 32;                              // head input blocks (two board bits x 16 channels each)
    // words (u32) of the image: head [part hi|lo][kb 32][lane 64][jj 8] halves, conv A [part][lane 64][jj 8] halves,
    // conv bias [q 4][r 4] (channel 4q + r, x 2^tc), head bias [q 4][r 4] (output 4q + r, x 2^(s1 + th); 12..15 zero),
    // scales: 2^(s1 - tc), 2^-(s1 + th), two unused
    static constexpr int HEAD_PART_WORDS = NKB * 64 * 4;        // 8,192
    static constexpr int CONV_W0 = 2 * HEAD_PART_WORDS;         // 16,384
    static constexpr int CONV_PART_WORDS = 64 * 4;              // 256
    static constexpr int CBIAS_W0 = CONV_W0 + 2 * CONV_PART_WORDS;
    static constexpr int HBIAS_W0 = CBIAS_W0 + 16;
    static constexpr int SCALE_W0 = HBIAS_W0 + 16;
    static constexpr int IMG_WORDS = SCALE_W0 + 4;              // 16,932 words = 67,728 B
    static constexpr uint32_t F16_ONE = 0x3C00u;
};
static_assert(ConvF16Geom::IMG_WORDS % 4 == 0, "the image is staged in 16-byte pieces");
static_assert((size_t)ConvF16Geom::IMG_WORDS * 4 <= (size_t)MlpGeom::IMG_FLOATS * 4, "the conv f16x2 image lives in the LDS region of the Connect4Net image");
static_assert(ConvF16Geom::IMG_WORDS <= F16Geom::IMG_WORDS, "the conv f16x2 image lives in the engine's f16x2 image buffer");

// Evaluates the network for the 16 positions of this wave's tile. Lane l = (j = l & 15, q = l >> 4) passes the bitboards of position
// j. Returns lane (j, q) register r = raw output 4q + r of position j DIVIDED by the image's out scale (multiply by the f32 at word
// SCALE_W0 + 1: an exact power of two) — the layout conv_tile16 returns.
SYN_DEV f32x4_ conv_f16x2_tile16(const uint32_t* __restrict__ img, int lane, uint64_t my, uint64_t op) {
    using G = ConvF16Geom;
    const int q = lane >> 4;
    const f16x8 cwh = as_f16x8(reinterpret_cast<const u32x4*>(img + G::CONV_W0)[lane]);
    const f16x8 cwl = as_f16x8(reinterpret_cast<const u32x4*>(img + G::CONV_W0 + G::CONV_PART_WORDS)[lane]);
    const f32x4_ cb = *reinterpret_cast<const f32x4_*>(img + G::CBIAS_W0 + 4 * q);
    f32x4_ hacc = *reinterpret_cast<const f32x4_*>(img + G::HBIAS_W0 + 4 * q);
    const float cs = bits_f32((uint32_t)__builtin_amdgcn_readfirstlane((int)img[G::SCALE_W0]));
    // the lane's eight taps 8q + jj as shifted boards (bit b = the tap's input for cell b; zero past tap 17)
    uint64_t T[8];
#pragma unroll
    for (int jj = 0; jj < 8; jj++) T[jj] = conv_tap_board(my, op, 8 * q + jj);
    const u32x4* hwh = reinterpret_cast<const u32x4*>(img) + lane;
    const u32x4* hwl = reinterpret_cast<const u32x4*>(img + G::HEAD_PART_WORDS) + lane;
    // four windows of 16 board bits (the last one's bit 63 is no cell: zero inputs, zero head weights)
#pragma unroll 1
    for (int w = 0; w < 4; w++) {
        // tap pair (2m, 2m + 1) of the window: bit c = cell 16w + c of tap 2m, bit 16 + c = the same cell of tap 2m + 1
        uint32_t P[4];
#pragma unroll
        for (int m = 0; m < 4; m++)
            P[m] = ((uint32_t)(T[2 * m] >> (16 * w)) & 0xFFFFu) | ((uint32_t)(T[2 * m + 1] >> (16 * w)) << 16);
        auto conv_cell = [&](int c) {
            u32x4 x;
#pragma unroll
            for (int m = 0; m < 4; m++) x[m] = ((P[m] >> c) & 0x10001u) * G::F16_ONE;   // two f16 inputs: 0 or 1.0
            const f16x8 xb = as_f16x8(x);
            f32x4_ acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(cwh, xb, cb, 0, 0, 0);
            return __builtin_amdgcn_mfma_f32_16x16x32_f16(cwl, xb, acc, 0, 0, 0);
        };
        // software-pipelined as conv_tile16: the conv MFMAs of cell c + 1 are issued before the split of cell c
        f32x4_ acc = conv_cell(0);
        u32x4 bh, bl, ah, al;
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if ((c & 1) == 0) {   // the head fragments of this cell pair, a cell ahead of their MFMAs
                const int kb = 8 * w + (c >> 1);
                ah = hwh[kb * 64];
                al = hwl[kb * 64];
            }
            f32x4_ nxt = acc;
            if (c < 15) nxt = conv_cell(c + 1);
            uint32_t h01, h23, l01, l23;
            f16x2_split_block(acc, cs, h01, h23, l01, l23);
            bh[2 * (c & 1)] = h01; bh[2 * (c & 1) + 1] = h23;
            bl[2 * (c & 1)] = l01; bl[2 * (c & 1) + 1] = l23;
            if (c & 1) {
                const f16x8 a_h = as_f16x8(ah), a_l = as_f16x8(al), x_h = as_f16x8(bh), x_l = as_f16x8(bl);
                hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, x_h, hacc, 0, 0, 0);
                hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, x_l, hacc, 0, 0, 0);
                hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_l, x_h, hacc, 0, 0, 0);
            }
            acc = nxt;
        }
    }
    return hacc;
}

// Batched Policy::eval with Connect4ConvNet in the f16x2 arithmetic: n positions -> logits[n][9], value[n][3] (the stand-alone form of
// the tile: a search's priors are this kernel's softmax)
template <int NT>
__global__ __launch_bounds__(NT) void policy_eval_conv_f16x2_kernel(const uint32_t* __restrict__ g_img,
                                                                    const unsigned long long* __restrict__ my_bb,
                                                                    const unsigned long long* __restrict__ op_bb, int n,
                                                                    float* __restrict__ logits, float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smemc16[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < ConvF16Geom::IMG_WORDS / 4; i += NT) reinterpret_cast<uint4*>(smemc16)[i] = reinterpret_cast<const uint4*>(g_img)[i];
    __syncthreads();
    const int ntiles = (n + 15) >> 4;
    const int j = lane & 15, q = lane >> 4;
    for (int tile = blockIdx.x * (NT / 64) + wave; tile < ntiles; tile += gridDim.x * (NT / 64)) {
        uint32_t img_off = 0;   // opaque per iteration: the image reads stay LDS reads next to their MFMAs
        asm volatile("" : "+v"(img_off));
        const uint32_t* img = smemc16 + img_off;
        const int pos = tile * 16 + j;
        const bool valid = pos < n;
        const uint64_t my = valid ? my_bb[pos] : 0ull, op = valid ? op_bb[pos] : 0ull;
        f32x4_ o = conv_f16x2_tile16(img, lane, my, op);
        const float os = reinterpret_cast<const float*>(img + ConvF16Geom::SCALE_W0)[1];
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] *= os;
        if (valid) {
            if (q < 2) {
#pragma unroll
                for (int r = 0; r < 4; r++) logits[(size_t)pos * 9 + q * 4 + r] = o[r];
            } else if (q == 2) {
                logits[(size_t)pos * 9 + 8] = o[0];
                float v0 = o[1], v1 = o[2], v2 = o[3];
                value_softmax(v0, v1, v2);
                value[(size_t)pos * 3 + 0] = v0;
                value[(size_t)pos * 3 + 1] = v1;
                value[(size_t)pos * 3 + 2] = v2;
            }
        }
    }
}

}  // namespace syn

// ====================================================================================================================================
// Host side: the per-checkpoint plan and the LDS image.  Plain C++, no device code.
namespace syn {

struct ConvF16Image {
    int tc = 0, s1 = 0, th = 0, out_exp = 0;   // conv weight scale, activation scale, head weight scale, raw = acc 2^out_exp
    double bound[2] = {0, 0};                  // conv activations (after ReLU), head outputs (unscaled)
    std::vector<uint32_t> words;               // ConvF16Geom::IMG_WORDS
};

inline int conv_f16x2_weight_exp(const float* w, size_t n, bool& ok) {
    double wmax = 0;
    for (size_t i = 0; i < n; i++) { if (!std::isfinite(w[i])) ok = false; wmax = std::fmax(wmax, std::fabs((double)w[i])); }
    int t = wmax > 0 ? 14 - f16x2_ceil_log2(wmax) : 0;
    return t > 40 ? 40 : t;
}

// blob order: conv.weight[16][2][3][3], conv.bias[16], head.weight[12][1008], head.bias[12] (convnet.cuh). Returns false when the
// checkpoint cannot be represented (non-finite parameters or scales outside the f32-safe window).
inline bool build_conv_f16x2_image(const float* blob, ConvF16Image& im) {
    using CG = ConvGeom;
    using G = ConvF16Geom;
    const float* cw = blob;
    const float* cb = blob + CG::CONV_W;
    const float* hw = cb + CG::C;
    const float* hb = hw + (size_t)CG::OUT * CG::FLAT;
    bool ok = true;
    im.tc = conv_f16x2_weight_exp(cw, CG::CONV_W, ok);
    im.th = conv_f16x2_weight_exp(hw, (size_t)CG::OUT * CG::FLAT, ok);
    for (int i = 0; i < CG::C; i++) if (!std::isfinite(cb[i])) ok = false;
    for (int i = 0; i < CG::OUT; i++) if (!std::isfinite(hb[i])) ok = false;
    if (!ok) return false;
    double ub[CG::C];
    double B0 = 0;
    for (int ch = 0; ch < CG::C; ch++) {
        double acc = (double)cb[ch];
        for (int t = 0; t < 18; t++) { const double w = (double)cw[ch * 18 + t]; acc += w > 0 ? w : 0.0; }
        ub[ch] = acc > 0 ? acc : 0.0;
        B0 = std::fmax(B0, ub[ch]);
    }
    double B1 = 0;
    for (int o = 0; o < CG::OUT; o++) {
        double acc = (double)hb[o];
        for (int i = 0; i < CG::FLAT; i++) { const double w = (double)hw[(size_t)o * CG::FLAT + i]; acc += (w > 0 ? w : 0.0) * ub[i / CG::HW]; }
        B1 = std::fmax(B1, std::fabs(acc));
    }
    im.bound[0] = B0;
    im.bound[1] = B1;
    im.s1 = 15 - f16x2_ceil_log2(std::fmax(B0, 1e-30));
    if (im.s1 > 24) im.s1 = 24;
    const int e_head = im.s1 + im.th;
    if (im.tc < -60 || im.tc > 60 || e_head < -60 || e_head > 60) return false;
    im.out_exp = -e_head;
    im.words.assign(G::IMG_WORDS, 0u);
    uint16_t* halfs = reinterpret_cast<uint16_t*>(im.words.data());
    float* fw = reinterpret_cast<float*>(im.words.data());
    auto split = [](float w, int e, uint16_t& hi, uint16_t& lo) {
        const float ws = std::ldexp(w, e);
        hi = f16x2_bits(ws);
        lo = f16x2_bits(ws - f16x2_value(hi));
    };
    for (int kb = 0; kb < G::NKB; kb++)
        for (int lane = 0; lane < 64; lane++)
            for (int jj = 0; jj < 8; jj++) {
                const int o = lane & 15, q = lane >> 4, ch = 4 * q + (jj & 3), b = 2 * kb + (jj >> 2);
                uint16_t hi = 0, lo = 0;
                if (o < CG::OUT && b < 63) split(hw[(size_t)o * CG::FLAT + ch * CG::HW + (b % 7) * 9 + b / 7], im.th, hi, lo);
                const size_t at = ((size_t)kb * 64 + lane) * 8 + jj;
                halfs[at] = hi;
                halfs[(size_t)2 * G::HEAD_PART_WORDS + at] = lo;
            }
    for (int lane = 0; lane < 64; lane++)
        for (int jj = 0; jj < 8; jj++) {
            const int ch = lane & 15, t = 8 * (lane >> 4) + jj;
            uint16_t hi = 0, lo = 0;
            if (t < 18) split(cw[ch * 18 + t], im.tc, hi, lo);
            halfs[(size_t)2 * G::CONV_W0 + lane * 8 + jj] = hi;
            halfs[(size_t)2 * (G::CONV_W0 + G::CONV_PART_WORDS) + lane * 8 + jj] = lo;
        }
    for (int i = 0; i < 16; i++) {
        fw[G::CBIAS_W0 + i] = std::ldexp(cb[i], im.tc);
        fw[G::HBIAS_W0 + i] = i < CG::OUT ? std::ldexp(hb[i], e_head) : 0.0f;
        if (!std::isfinite(fw[G::CBIAS_W0 + i]) || !std::isfinite(fw[G::HBIAS_W0 + i])) return false;   // a bias outside the window
    }
    fw[G::SCALE_W0 + 0] = std::ldexp(1.0f, im.s1 - im.tc);
    fw[G::SCALE_W0 + 1] = std::ldexp(1.0f, im.out_exp);
    return true;
}

}  // namespace syn
