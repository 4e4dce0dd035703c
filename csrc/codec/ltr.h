// Long-term reference cache: the policy that decides which reconstructed pictures a
// stream keeps beyond its sliding window, when a slice predicts from one of them, and
// the model of the decoder's reference bookkeeping that keeps the stream inside its DPB.
// POD state and SK_HD functions only (frame numbers are the codec's picture counter modulo
// `fn_mask + 1`), so the CPU back end and the GPU frame graph run the same code.
//
// A stream is what owns a decoder: a stripe in striped mode, the picture in full-frame
// mode. All quantities are integers, so both back ends decide identically.
//
// LtrConfig is a session's cache: the slot count (0: off), the expiry age and the LtrMode,
// which says how the codec names a cached picture (H.264: second reference and marking
// model; HEVC: exclusive, RPS; AV1: exclusive, buffer map, tile rows). It is derived once,
// by ltr_config_of (h264_encoder.h). Entry points, one of each for all modes:
//   ltr_decide   the stream's decision for one frame, before motion search
//   ltr_commit   the stream's state after its picture was coded; the mode selects the tail
//   ltr_av1_frame_bufs   the buffers an AV1 frame header names
// ltr_stream_decide, ltr_stream_commit and ltr_ref1_mbs (h264_encoder.h) wrap them with what
// a stream's SliceTasks say; every back end calls those.
#pragma once
#include <stdint.h>
#include "sk_common.h"

namespace sk {
namespace ltr {

constexpr int kLtrMaxSlots = 8;    // EncoderConfig::ltr_slots upper bound
constexpr int kLtrSettle = 8;      // consecutive quiet frames after which a stream's content counts as settled
constexpr int kLtrQuietDen = 16;   // quiet frame: dirty MBs < 1/16 of the stream's MBs
constexpr int kLtrLargeDen = 4;    // large change: dirty MBs >= 1/4 of the stream's MBs
constexpr int kLtrSadCols = 1 + kLtrMaxSlots;   // per slice: SAD against the current reference, then each slot

// How the codec names a cached picture.
enum LtrMode : int32_t {
    LTR_SECOND_REF = 0,   // H.264: the slot is reference index 1, next to the previous picture; marking model (8.2.5)
    LTR_RPS = 1,          // HEVC: exclusive (a matched slice predicts from its slot alone), POC table, expiry
    LTR_BUFMAP = 2,       // AV1: exclusive, the decoder's buffer map, the tile row is the decision unit
};

// A session's cache. slots == 0: off, and the other fields are 0.
struct LtrConfig {
    int32_t slots;         // pictures kept per stream
    int32_t mode;          // LtrMode
    int32_t unit_slices;   // LTR_BUFMAP: front-end slices in one tile row
    int32_t max_age;       // LTR_RPS: expiry age in pictures (ltr_expire)
};

// Per stream, carried from frame to frame (and in the version-4 state blob).
struct LtrState {
    int32_t quiet_run;             // consecutive quiet frames up to now
    int32_t cur_slot;              // slot that holds the stream's current content, -1: none
    int32_t clock;                 // frames with a large change seen (the stamps' time base)
    int32_t valid;                 // bit j: slot j holds a picture == long-term frame index j in use
    int32_t stamp[kLtrMaxSlots];   // clock of the slot's last store or match
    // model of the decoder's marking state (8.2.5): short-term frame_nums, oldest first
    int32_t n_st;
    int32_t st_fn[kLtrMaxSlots + 1];
    int32_t pad[2];
};
static_assert(sizeof(LtrState) == 96, "LtrState layout");

enum LtrFlags : int32_t { LTR_GATED = 1, LTR_DRIFT = 2 };

// Per slice and frame: what the policy decided (parallel to SliceTask).
struct LtrTask {
    int32_t slot;         // cached picture this slice predicts from (reference index 1), -1: none
    int32_t store_slot;   // the stream's previous picture becomes long-term index store_slot, -1: no store
    int32_t mmco1;        // difference_of_pic_nums_minus1 of the short-term picture to drop first, -1: none
    int32_t flags;        // LtrFlags of the stream's frame
    int32_t ref1_mbs;     // macroblocks of the slice coded from `slot` (set with the scene-cut decision)
    int32_t pad[3];
};
static_assert(sizeof(LtrTask) == 32, "LtrTask layout");

SK_HD void ltr_state_reset(LtrState& st) {
    st.quiet_run = 0;
    st.cur_slot = -1;
    st.clock = 0;
    st.valid = 0;
    for (int j = 0; j < kLtrMaxSlots; j++) st.stamp[j] = 0;
    st.n_st = 0;
    for (int j = 0; j <= kLtrMaxSlots; j++) st.st_fn[j] = 0;
    st.pad[0] = st.pad[1] = 0;
}

SK_HD void ltr_task_reset(LtrTask& t) {
    t.slot = t.store_slot = t.mmco1 = -1;
    t.flags = t.ref1_mbs = 0;
    t.pad[0] = t.pad[1] = t.pad[2] = 0;
}

SK_HD bool ltr_quiet(int dirty, int mbs) { return dirty * kLtrQuietDen < mbs; }
SK_HD bool ltr_large(int dirty, int mbs) { return dirty * kLtrLargeDen >= mbs; }
SK_HD int ltr_popcount(int v) {
    int n = 0;
    for (int j = 0; j < kLtrMaxSlots; j++) n += (v >> j) & 1;
    return n;
}

// Slot a slice predicts from: the valid slot with the smallest zero-vector SAD if it
// beats the current reference (ties: lowest index), else -1. sad[0] is the SAD against
// the current reference, sad[1 + j] against slot j.
SK_HD int ltr_match(int valid, int slots, const uint32_t* sad) {
    int best = -1;
    uint32_t bs = sad[0];
    for (int j = 0; j < slots; j++)
        if (((valid >> j) & 1) && sad[1 + j] < bs) {
            bs = sad[1 + j];
            best = j;
        }
    return best;
}

// Slot the previous picture is stored into: the lowest free one, else the least
// recently used (ties: lowest index).
SK_HD int ltr_store_slot(const LtrState& st, int slots) {
    for (int j = 0; j < slots; j++)
        if (!((st.valid >> j) & 1)) return j;
    int best = 0;
    for (int j = 1; j < slots; j++)
        if (st.stamp[j] < st.stamp[best]) best = j;
    return best;
}

// The stream's decision for one frame, before motion search. `dirty` of the stream's
// `mbs` macroblocks changed; `planned_p`: the picture is planned as P (no key frame);
// slices [s0, s1) belong to the stream and slice s may predict when p_slice(s). `sad`
// holds kLtrSadCols sums per slice and is only read on a gated frame. Fills lt[s0..s1)
// and updates the quiet run, the clock and the stamps; the marking model moves in
// ltr_commit.
template <class IsP>
SK_HD void ltr_decide(int slots, LtrState& st, int dirty, int mbs, bool planned_p, int frame_num, int fn_mask,
                      int s0, int s1, IsP p_slice, const uint32_t* sad, LtrTask* lt) {
    const bool settled = st.quiet_run >= kLtrSettle;
    const bool quiet = ltr_quiet(dirty, mbs), large = ltr_large(dirty, mbs);
    st.quiet_run = quiet ? st.quiet_run + 1 : 0;
    for (int s = s0; s < s1; s++) ltr_task_reset(lt[s]);
    int flags = 0;
    if (large && planned_p) flags = LTR_GATED;
    else if (!quiet) flags = LTR_DRIFT;
    int store = -1, mmco1 = -1;
    if (flags & LTR_GATED) {
        st.clock++;
        for (int s = s0; s < s1; s++) {
            if (!p_slice(s)) continue;
            const int j = ltr_match(st.valid, slots, sad + (size_t)s * kLtrSadCols);
            lt[s].slot = j;
            if (j >= 0) st.stamp[j] = st.clock;
        }
        if (st.cur_slot >= 0) {
            st.stamp[st.cur_slot] = st.clock;
        } else if (settled && st.n_st > 0) {
            store = ltr_store_slot(st, slots);
            st.stamp[store] = st.clock;
            // DPB after marking: the short-term pictures (the previous one leaves, this one
            // joins) and the long-term ones; over max_num_ref_frames = 1 + slots the oldest
            // short-term picture goes first (MMCO 1)
            const int n_lt = ltr_popcount(st.valid) + (((st.valid >> store) & 1) ? 0 : 1);
            if (st.n_st + n_lt > 1 + slots && st.n_st >= 2)
                mmco1 = ((frame_num - st.st_fn[0]) & fn_mask) - 1;
        }
    }
    for (int s = s0; s < s1; s++) {
        lt[s].store_slot = store;
        lt[s].mmco1 = mmco1;
        lt[s].flags = flags;
    }
}

// ---- LTR_RPS (HEVC) -------------------------------------------------------------------
// A matched slice predicts from its slot alone (reference index 0 of a one-entry list), so
// the slice keeps one reference and every unit coded as P counts for the slot. An RPS names
// every picture the decoder keeps, so no marking model is needed; the free fields hold
// picture order counts instead: st_fn[j] = POC LSBs (16 bits) of slot j's picture, n_st = 1
// once a previous picture exists (the store condition of ltr_decide), mmco1 stays -1.
constexpr int kLtrPocMask = 0xffff;
constexpr int kLtrMaxAge = 32768;   // default and upper bound of the expiry age

SK_HD int ltr_clip_max_age(int n) { return n < 2 ? 2 : (n > kLtrMaxAge ? kLtrMaxAge : n); }

// Expiry, at the start of a picture's decision (`poc`: its POC LSBs): a slot whose picture
// is max_age or more pictures old leaves the cache. Checked on every coded picture, so no
// age is stepped over and all POCs a decoder holds span less than 2^16: long-term entries
// need no MSB.
SK_HD void ltr_expire(int slots, LtrState& st, int poc, int max_age) {
    for (int j = 0; j < slots; j++)
        if (((st.valid >> j) & 1) && ((poc - st.st_fn[j]) & kLtrPocMask) >= max_age) {
            st.valid &= ~(1 << j);
            if (st.cur_slot == j) st.cur_slot = -1;
        }
}

// ref1_mbs of a slice once its scene-cut decision is known (`coded_p`: it is coded as P;
// `counted_ref1`: its macroblocks whose vector points at reference index 1). Exclusive
// modes: all of its `slice_mbs` units when it matched a slot; LTR_BUFMAP set that with the
// decision already (ltr_av1_reduce: clean slices of a matched tile row count too).
SK_HD int ltr_ref1_mbs(const LtrConfig& c, const LtrTask& t, bool coded_p, int slice_mbs, int counted_ref1) {
    if (c.mode == LTR_BUFMAP) return t.ref1_mbs;
    if (c.mode == LTR_RPS) return t.slot >= 0 && coded_p ? slice_mbs : 0;
    return coded_p ? counted_ref1 : 0;   // the stream's cur_slot (ltr_commit)
}

// ---- LTR_BUFMAP (AV1) -----------------------------------------------------------------
// An AV1 decoder owns eight reference buffers and a frame header names the ones it reads
// and writes, so a cached picture is a buffer that later frames leave alone. A picture
// cannot be moved after it was decoded: storing the previous picture into slot k means
// that its buffer becomes slot k's and the new picture goes elsewhere. The decision unit is
// a tile row (a run of `unit_slices` front-end slices) and a frame reads one slot at most.
// The free fields hold the map: st_fn[j] = buffer of slot j (j < slots <= 7),
// st_fn[kLtrMaxSlots] = buffer of the previous picture, n_st = 1 once one exists.
constexpr int kLtrAv1MaxSlots = 7;   // eight buffers: the previous picture and the slots

SK_HD int ltr_av1_last_buf(const LtrState& st) { return st.st_fn[kLtrMaxSlots]; }

// Buffer the picture being coded is written to (refresh_frame_flags = 1 << it), from the
// state before its commit: the previous picture's own buffer without a store; with one, the
// lowest buffer that neither the previous picture nor a slot other than store_slot holds
// (store_slot's old buffer is free again).
SK_HD int ltr_av1_new_buf(int slots, const LtrState& st, int store_slot) {
    const int last = ltr_av1_last_buf(st);
    if (store_slot < 0) return last;
    int used = 1 << last;
    for (int j = 0; j < slots; j++)
        if (j != store_slot && ((st.valid >> j) & 1)) used |= 1 << st.st_fn[j];
    int b = 0;
    while ((used >> b) & 1) b++;   // 1 + slots <= 8 buffers are in use, so one below 8 is free
    return b;
}

// The SADs of the slices of one unit summed and written back to each of them, so that
// ltr_match gives every slice of a tile row the same slot.
SK_HD void ltr_sum_units(int slots, int valid, int s0, int s1, int unit_slices, uint32_t* sad) {
    for (int u0 = s0; u0 < s1; u0 += unit_slices) {
        const int u1 = u0 + unit_slices < s1 ? u0 + unit_slices : s1;
        for (int c = 0; c <= slots; c++) {
            if (c > 0 && !((valid >> (c - 1)) & 1)) continue;
            uint32_t sum = 0;
            for (int s = u0; s < u1; s++) sum += sad[(size_t)s * kLtrSadCols + c];
            for (int s = u0; s < u1; s++) sad[(size_t)s * kLtrSadCols + c] = sum;
        }
    }
}

// The one slot a frame reads: the slot matched by the most units over the tile rows
// (`unit_slices` slices each, `units(s)`: units of slice s), ties to the lowest index; the
// rows that matched another slot fall back to the previous picture. Sets ref1_mbs of every
// slice: all of its units where it keeps a slot. Returns the slot, -1: none.
template <class Units>
SK_HD int ltr_av1_reduce(int slots, int s0, int s1, Units units, LtrTask* lt) {
    int best = -1, best_n = 0;
    for (int j = 0; j < slots; j++) {
        int n = 0;
        for (int s = s0; s < s1; s++)
            if (lt[s].slot == j) n += units(s);
        if (n > best_n) {
            best_n = n;
            best = j;
        }
    }
    for (int s = s0; s < s1; s++) {
        if (lt[s].slot != best) lt[s].slot = -1;
        lt[s].ref1_mbs = lt[s].slot >= 0 ? units(s) : 0;
    }
    return best;
}

// The buffers an inter frame's header names, from the map before the frame's commit and the
// decisions of its `ns` slices: the one it is written to, the previous picture's (LAST) and
// the frame's slot's (LAST2; the previous picture's again without a slot).
struct LtrAv1Bufs {
    int refresh;   // refresh_frame_flags
    int last, last2;
};
SK_HD LtrAv1Bufs ltr_av1_frame_bufs(const LtrConfig& c, const LtrState& st, const LtrTask* lt, int ns) {
    int slot = -1;
    for (int s = 0; s < ns; s++) slot = sk_max(slot, lt[s].slot);   // one slot per frame (ltr_av1_reduce)
    const int last = ltr_av1_last_buf(st);
    return LtrAv1Bufs{1 << ltr_av1_new_buf(c.slots, st, lt[0].store_slot), last, slot >= 0 ? st.st_fn[slot] : last};
}

// ---- all modes ------------------------------------------------------------------------
// After the stream's picture was coded (`coded`: it produced a picture at all; `idr`: an
// IDR picture or a key frame; `fn`: its frame_num, LTR_RPS: its POC LSBs): the
// current-content slot from the per-slice reference counts, then the decoder's bookkeeping
// in the mode's terms.
SK_HD void ltr_commit(const LtrConfig& c, LtrState& st, bool coded, bool idr, int fn, int mbs, int s0, int s1,
                      const LtrTask* lt) {
    if (!coded) return;
    if (idr) {   // empties the cache; one previous picture (H.264: short-term, frame_num 0; AV1: in buffer 0)
        const int q = st.quiet_run;
        ltr_state_reset(st);
        st.quiet_run = q;
        st.n_st = 1;
        return;
    }
    const LtrTask& f = lt[s0];
    if (f.flags & LTR_GATED) {
        st.cur_slot = -1;
        for (int j = c.slots - 1; j >= 0; j--) {
            int cnt = 0;
            for (int s = s0; s < s1; s++)
                if (lt[s].slot == j) cnt += lt[s].ref1_mbs;
            if (2 * cnt >= mbs) st.cur_slot = j;
        }
        if (st.cur_slot >= 0 && st.cur_slot == f.store_slot) st.cur_slot = -1;   // the slot now holds the previous content
    } else if (f.flags & LTR_DRIFT) {
        st.cur_slot = -1;   // neither quiet nor a switch: the content moved away from the slot's
    }
    if (c.mode == LTR_SECOND_REF) {   // what the decoder does with the picture's dec_ref_pic_marking()
        if (f.store_slot >= 0) {
            if (f.mmco1 >= 0) {   // MMCO 1: the oldest short-term picture
                for (int k = 1; k < st.n_st; k++) st.st_fn[k - 1] = st.st_fn[k];
                st.n_st--;
            }
            st.n_st--;            // MMCO 3: the previous picture (the newest short-term one) turns long-term
            st.valid |= 1 << f.store_slot;
        } else if (st.n_st + ltr_popcount(st.valid) >= 1 + c.slots && st.n_st > 0) {
            for (int k = 1; k < st.n_st; k++) st.st_fn[k - 1] = st.st_fn[k];   // sliding window (8.2.5.3)
            st.n_st--;
        }
        st.st_fn[st.n_st++] = fn;
        return;
    }
    if (f.store_slot >= 0) {
        if (c.mode == LTR_RPS) {   // the stored picture is the one before this
            st.st_fn[f.store_slot] = (fn - 1) & kLtrPocMask;
        } else {
            const int nb = ltr_av1_new_buf(c.slots, st, f.store_slot);   // read before the map moves
            st.st_fn[f.store_slot] = ltr_av1_last_buf(st);   // the previous picture stays where it is
            st.st_fn[kLtrMaxSlots] = nb;
        }
        st.valid |= 1 << f.store_slot;
    }
    st.n_st = 1;
}

}  // namespace ltr
}  // namespace sk
