// agc.hip — the AGC stage (sdrg_engine_agc_*): a block stage (block_stage.h has the positions, the three launches and
// the state's layout) whose statistic is the block's mean power, by the squelch's adjacent-pair tree, or its peak power.
// Each completed block's statistic moves one gain per stream by an attack / hang / decay law, and block b is multiplied
// by a ramp from gain[b - 2] to gain[b - 1], so the gain is continuous across the seams and no decision reaches back into
// the block that produced it (include/sdrg.h).  What is the AGC's own:
//   step    G, the hang counter and the attack count; blk keeps gain[k], the gain after each block.  The state's words
//           are {G, G_prev, hang, P_last}; the record has both dB, of G and of P_last + 1e-20.
//   pass    a sample passes under the ramp of its block (g1 = blk[k - 1], g0 = blk[k - 2], or the old state's G and
//           G_prev for the call's first two blocks).
// Compiled with -ffp-contract=off: every product, sum, quotient and root is rounded on its own (`/` and sqrtf are the
// compiler's correctly rounded sequences: tests/cpp/demod_math.hip).
#include "block_stage.h"

namespace sdrg {
namespace {

struct AgcLaw {
    using Params = AgcParams;
    using Old = float2;     // {G, G_prev} before the call
    using Weight = float2;  // the gains at the two ends of a block's ramp

    float G, Gp, Pl = 0.0f;
    int hang = 0, attacks = 0;
    const float target, max_gain, floor_thr, aa, ad;
    const bool whole_a, whole_d;
    const int H;

    __device__ explicit AgcLaw(const Params &p)
        : G(p.init_gain), Gp(p.init_gain), target(p.target), max_gain(p.max_gain), floor_thr(p.floor_thr),
          aa(p.alpha_a), ad(p.alpha_d), whole_a(p.alpha_a == 1.0f), whole_d(p.alpha_d == 1.0f), H(p.hang) {}

    __device__ void unpack(float4 s) { G = s.x, Gp = s.y, hang = __float_as_int(s.z), Pl = s.w; }

    __device__ float4 pack() const { return make_float4(G, Gp, __int_as_float(hang), Pl); }

    __device__ float step(float P) {
        Gp = G;
        Pl = P;
        if (P < floor_thr) return G;  // the hold: neither the gain nor the hang counter moves
        const float a = sqrtf(P);
        const float want = fminf(target / a, max_gain);
        const float d = want - G;
        if (want < G) {
            G = whole_a ? want : G + aa * d;
            hang = H;
            attacks++;
        } else if (hang > 0) {
            hang = hang - 1;
        } else {
            G = whole_d ? want : G + ad * d;
        }
        return G;
    }

    __device__ sdrg_agc_record record(const glibc::LogfEntry *tab) const {
        sdrg_agc_record r;
        r.gain = G;
        r.gain_db = 20.0f * glibc::log10f_fast(G, tab);
        r.level_db = 10.0f * glibc::log10f_fast(Pl + 1e-20f, tab);
        r.attacks = attacks;
        return r;
    }

    static __device__ Old old(const Params &p, const float *state) {
        float2 old = make_float2(p.init_gain, p.init_gain);
        if (!p.fresh) old = *reinterpret_cast<const float2 *>(state);
        return old;
    }

    // {gain[-2], gain[-1]} counted from the call's block k
    static __device__ Weight fetch(int k, Old old, const float *col, size_t B) {
        const float g1 = k >= 1 ? col[(size_t)(k - 1) * B] : old.x;
        const float g0 = k >= 2 ? col[(size_t)(k - 2) * B] : (k == 1 ? old.x : old.y);
        return make_float2(g0, g1);
    }

    static __device__ float2 apply(float2 z, int i, Weight g, const Params &p) {
        const float t = (float)(i + 1) * p.inv_block;
        const float d = g.y - g.x;
        const float w = g.x + d * t;
        return make_float2(z.x * w, z.y * w);
    }
};

}  // namespace

hipError_t launch_agc(const float *chan, int n_streams, const AgcParams &p, float *out, hipStream_t stream) {
    if (p.detector == SDRG_AGC_DET_PEAK) return launch_block_stage<AgcLaw, true>(chan, n_streams, p, out, stream);
    if (p.detector == SDRG_AGC_DET_MEAN) return launch_block_stage<AgcLaw, false>(chan, n_streams, p, out, stream);
    return n_streams <= 0 ? hipSuccess : hipErrorInvalidValue;
}

}  // namespace sdrg
