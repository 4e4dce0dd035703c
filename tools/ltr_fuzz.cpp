// Host-only check of the long-term cache's shared entry points (codec/ltr.h, codec/h264_encoder.h):
// drives plan_stripe -> ltr_stream_decide -> ltr_ref1_mbs -> ltr_stream_commit -> commit_* in all
// three modes over random frames (dirty counts, SADs, key frames, scene cuts, uncoded stripes) and
// checks the invariants the code's comments state. Build with the sanitizers and run:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc/codec \
//       tools/ltr_fuzz.cpp -o /tmp/ltr_fuzz && /tmp/ltr_fuzz [frames] [seed]
#include <stdio.h>
#include <random>
#include <vector>
#include "h264_encoder.h"

using namespace sk;
using namespace sk::h264;

static int fails = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fails++;                                      \
            printf("FAIL %s: ", #cond);                   \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

static void check_state(const ltr::LtrConfig& c, const ltr::LtrState& st, const char* what, int frame) {
    CHECK(st.cur_slot >= -1 && st.cur_slot < c.slots, "%s frame %d cur_slot %d", what, frame, st.cur_slot);
    CHECK((st.valid >> c.slots) == 0, "%s frame %d valid %x", what, frame, st.valid);
    CHECK(st.cur_slot < 0 || ((st.valid >> st.cur_slot) & 1), "%s frame %d cur_slot %d not valid", what, frame, st.cur_slot);
    if (c.mode == ltr::LTR_SECOND_REF) {
        CHECK(st.n_st >= 0 && st.n_st + ltr::ltr_popcount(st.valid) <= 1 + c.slots, "%s frame %d n_st %d valid %x", what,
              frame, st.n_st, st.valid);
    } else if (c.mode == ltr::LTR_BUFMAP) {
        int used = 0;
        for (int j = 0; j <= ltr::kLtrMaxSlots; j++) {
            if (j < ltr::kLtrMaxSlots && !((st.valid >> j) & 1)) continue;
            const int b = st.st_fn[j];
            CHECK(b >= 0 && b < 8, "%s frame %d buffer %d of %d", what, frame, b, j);
            CHECK(!((used >> b) & 1), "%s frame %d buffer %d twice", what, frame, b);
            used |= 1 << (b & 7);
        }
    }
}

static void run(int codec, int fullframe, int slots, int frames, uint32_t seed) {
    EncoderConfig ec;
    ec.width = 208;
    ec.height = 112;
    ec.stripe_height = 32;
    ec.fullframe = fullframe;
    ec.codec = codec;
    ec.ltr_slots = slots;
    ec.use_paint_over = 0;
    if (ltr_config_error(ec)) {
        printf("FAIL config: %s\n", ltr_config_error(ec));
        fails++;
        return;
    }
    char what[64];
    snprintf(what, sizeof what, "codec %d ff %d slots %d", codec, fullframe, slots);
    ltr::LtrConfig c = ltr_config_of(ec);
    if (c.mode == ltr::LTR_RPS) c.max_age = 24;   // pictures: slots expire within the run
    const PlanConfig pc = plan_config(ec);
    Geometry g;
    g.init(ec);
    const int ns = g.num_slices;
    std::mt19937 rng(seed);
    auto rnd = [&](int n) { return (int)(rng() % (uint32_t)n); };
    std::vector<StripeState> ss(ns + 1);
    ltr::LtrState z;
    ltr::ltr_state_reset(z);
    std::vector<ltr::LtrState> ls(ns + 1, z);
    std::vector<ltr::LtrTask> lt(ns);
    std::vector<SliceTask> tasks(ns);
    std::vector<uint32_t> sad((size_t)ns * ltr::kLtrSadCols);
    long stores = 0, matches = 0;
    int quiet_left = 0;
    for (int f = 0; f < frames; f++) {
        if (rnd(40) == 0) {   // key frame request
            for (auto& s : ss) s.need_idr = true;
        }
        // runs of quiet frames, so streams settle; between them large changes (6..8) and drift (9)
        if (quiet_left > 0) quiet_left--;
        else if (rnd(3) == 0) quiet_left = 6 + rnd(8);
        const int regime = quiet_left > 0 ? 0 : 6 + rnd(4);
        std::vector<int> dirty(ns);
        for (int s = 0; s < ns; s++) {
            const int n = g.slice_rows(s) * g.mb_w;
            dirty[s] = regime < 6 ? 0 : regime < 9 ? n / 4 + rnd(n - n / 4 + 1) : rnd(n / 4 + 1);
            if (regime >= 6 && rnd(8) == 0) dirty[s] = 0;   // a stripe that stays clean
            plan_stripe(pc, ss[s], ss[ns], dirty[s] > 0, g.slice_first_row(s), g.slice_rows(s), g.mb_h, tasks[s]);
        }
        for (auto& x : sad) x = rng() & 0xffffff;
        for (int k = 0; k < (fullframe ? 1 : ns); k++) {
            const int s0 = fullframe ? 0 : k, s1 = fullframe ? ns : k + 1;
            ltr::LtrState& st = ls[fullframe ? ns : k];
            int nd = 0, n = 0;
            bool anyp = false, key = false;
            for (int s = s0; s < s1; s++) {
                nd += dirty[s];
                n += tasks[s].num_rows * g.mb_w;
                anyp |= tasks[s].action == ACT_P;
                key |= tasks[s].action == ACT_I;
            }
            const bool gated = anyp && !key && ltr::ltr_large(nd, n) && st.valid;
            const int valid_before = st.valid;
            ltr_stream_decide(c, st, tasks.data(), s0, s1, nd, g.mb_w, gated, sad.data(), lt.data());
            check_state(c, st, what, f);
            int frame_slot = -1;
            for (int s = s0; s < s1; s++) {
                CHECK(lt[s].slot >= -1 && lt[s].slot < c.slots, "%s frame %d slot %d", what, f, lt[s].slot);
                CHECK(lt[s].slot < 0 || ((valid_before >> lt[s].slot) & 1), "%s frame %d slot %d not valid", what, f, lt[s].slot);
                CHECK(lt[s].store_slot >= -1 && lt[s].store_slot < c.slots, "%s frame %d store %d", what, f, lt[s].store_slot);
                CHECK(tasks[s].num_refs == (c.mode == ltr::LTR_SECOND_REF && lt[s].slot >= 0 ? 2 : 1), "%s frame %d num_refs", what, f);
                if (lt[s].slot >= 0) {
                    matches++;
                    CHECK(c.mode != ltr::LTR_BUFMAP || frame_slot < 0 || frame_slot == lt[s].slot, "%s frame %d two slots", what, f);
                    frame_slot = lt[s].slot;
                }
            }
            stores += lt[s0].store_slot >= 0;
        }
        // scene cuts, the picture's key decision, ref1_mbs
        bool any_i = false;
        for (int s = 0; s < ns; s++) {
            SliceTask& t = tasks[s];
            t.final_action = t.action;
            if (t.action == ACT_P && t.allow_scenecut && rnd(12) == 0) t.final_action = ACT_I;
            any_i |= t.final_action == ACT_I;
        }
        if (codec == 2 && any_i)
            for (int s = 0; s < ns; s++) tasks[s].final_action = ACT_I;
        for (int s = 0; s < ns; s++) {
            const SliceTask& t = tasks[s];
            if (t.action != ACT_P) continue;
            const int n = t.num_rows * g.mb_w;
            lt[s].ref1_mbs = ltr::ltr_ref1_mbs(c, lt[s], t.final_action == ACT_P, n, lt[s].slot >= 0 ? rnd(n + 1) : 0);
            CHECK(lt[s].ref1_mbs >= 0 && lt[s].ref1_mbs <= n, "%s frame %d ref1_mbs %d", what, f, lt[s].ref1_mbs);
        }
        bool idr = true;
        for (int s = 0; s < ns; s++) idr &= tasks[s].final_action == ACT_I && tasks[s].idr_on_intra;
        if (c.mode == ltr::LTR_BUFMAP && !idr) {
            const ltr::LtrAv1Bufs b = ltr::ltr_av1_frame_bufs(c, ls[ns], lt.data(), ns);
            CHECK(b.last >= 0 && b.last < 8 && b.last2 >= 0 && b.last2 < 8, "%s frame %d bufs %d %d", what, f, b.last, b.last2);
            CHECK(b.refresh > 0 && b.refresh < 256 && !(b.refresh & (b.refresh - 1)), "%s frame %d refresh %x", what, f, b.refresh);
        }
        for (int k = 0; k < (fullframe ? 1 : ns); k++) {
            ltr_stream_commit(c, ls[fullframe ? ns : k], tasks.data(), lt.data(), k, fullframe ? ns : k + 1, g.mb_w,
                              g.num_mbs(), fullframe != 0, idr);
            check_state(c, ls[fullframe ? ns : k], what, f);
        }
        if (fullframe) commit_picture(ss[ns], idr, pc.num_refs);
        else
            for (int s = 0; s < ns; s++) commit_stripe(ss[s], tasks[s].final_action, pc.num_refs, tasks[s].idr_on_intra != 0);
    }
    printf("%s: %d frames, %ld stores, %ld matched slices\n", what, frames, stores, matches);
    CHECK(stores > 0 && matches > 0, "%s: the run exercised nothing", what);
}

int main(int argc, char** argv) {
    const int frames = argc > 1 ? atoi(argv[1]) : 600;
    const uint32_t seed = argc > 2 ? (uint32_t)atoi(argv[2]) : 1;
    for (int slots : {1, 2, 7}) {
        run(0, 0, slots, frames, seed);
        run(0, 1, slots, frames, seed + 1);
        run(1, 1, slots, frames, seed + 2);
        run(2, 1, slots, frames, seed + 3);
    }
    printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails != 0;
}
