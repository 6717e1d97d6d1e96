// squelch.hip — the squelch stage (sdrg_engine_squelch_*): a block stage (block_stage.h has the positions, the three
// launches and the state's layout) whose statistic is the block's mean power.  Each completed block's mean power updates
// a smoothed level, a hysteresis gate with a hang time decides from it how the next block passes, and a record reports
// level and gate (include/sdrg.h).  What is the squelch's own:
//   step    the level, the gate and the hang counter; blk keeps the code of the block after each (2 * the gate before +
//           the gate after).  The state's words are {L, open, hang, code}; the record's dB is 10 log10(L + 1e-20).
//   pass    a sample passes under the code of its block (block 0 of the call: the state's; block k: blk[k - 1]): whole,
//           zero, or under a ramp up or down over the block.
// Compiled with -ffp-contract=off: every product and sum is rounded on its own.
#include "block_stage.h"

namespace sdrg {
namespace {

struct SquelchLaw {
    using Params = SquelchParams;
    using Old = int;     // the code of the block in progress
    using Weight = int;  // a block's code

    float L = 0.0f;
    int open = 0, hang = 0, code = 0, open_blocks = 0;
    const float beta, open_thr, close_thr;
    const bool whole;
    const int H;

    __device__ explicit SquelchLaw(const Params &p)
        : beta(p.beta), open_thr(p.open_thr), close_thr(p.close_thr), whole(p.beta == 1.0f), H(p.hang) {}

    __device__ void unpack(float4 s) {
        L = s.x, open = __float_as_int(s.y), hang = __float_as_int(s.z), code = __float_as_int(s.w);
    }

    __device__ float4 pack() const {
        return make_float4(L, __int_as_float(open), __int_as_float(hang), __int_as_float(code));
    }

    __device__ float step(float P) {
        if (whole) {
            L = P;
        } else {
            const float d = P - L;
            L = L + beta * d;
        }
        const int was = open;
        if (open) {
            if (L >= close_thr)
                hang = H;
            else if (hang > 0)
                hang = hang - 1;
            else
                open = 0;
        } else if (L >= open_thr) {
            open = 1, hang = H;
        }
        code = 2 * was + open;
        open_blocks += open;
        return __int_as_float(code);
    }

    __device__ sdrg_squelch_record record(const glibc::LogfEntry *tab) const {
        sdrg_squelch_record r;
        r.level = L;
        r.level_db = 10.0f * glibc::log10f_fast(L + 1e-20f, tab);
        r.open = open;
        r.open_blocks = open_blocks;
        return r;
    }

    static __device__ Old old(const Params &p, const float *state) {
        return p.fresh ? 0 : __float_as_int(state[BLOCK_STATE_HEAD - 1]);
    }

    static __device__ Weight fetch(int k, Old code0, const float *col, size_t B) {
        return k == 0 ? code0 : __float_as_int(col[(size_t)(k - 1) * B]);
    }

    static __device__ float2 apply(float2 z, int i, Weight code, const Params &p) {
        if (code == 3) return z;
        if (code == 0) return make_float2(0.0f, 0.0f);
        const float w = (float)(code == 1 ? i + 1 : p.block - 1 - i) * p.inv_block;
        return make_float2(z.x * w, z.y * w);
    }
};

}  // namespace

hipError_t launch_squelch(const float *chan, int n_streams, const SquelchParams &p, float *out, hipStream_t stream) {
    return launch_block_stage<SquelchLaw, false>(chan, n_streams, p, out, stream);
}

}  // namespace sdrg
