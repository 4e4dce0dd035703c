"""Hand-worked vectors for the test decoder's reference picture marking and list code
(models/h264/decoder.py RefMarking), which checks every long-term-reference stream of the
encoder tests. Expected values are worked from ITU-T H.264 (frames only: PicNum =
FrameNumWrap, LongTermPicNum = LongTermFrameIdx), not from the encoders: 8.2.4.1 picture
numbers, 8.2.4.2.1 initial list, 8.2.4.3 list modification, 8.2.5.3 sliding window, 8.2.5.4
adaptive marking. Frames are named by frame_num (short-term) or "LTi" (long-term index i)."""
import pytest

from selkies_gstreamer_amd.models.h264 import decoder as D
from selkies_gstreamer_amd.models.h264.decoder import BitstreamError, RefFrame, RefMarking

MAXFN = 16   # MaxFrameNum (log2_max_frame_num = 4) keeps the wrap cases small


def _dpb(short=(), long=(), max_lt=None):
    m = RefMarking()
    m.short = [RefFrame(fn) for fn in short]
    m.long = [RefFrame(fn, long_term_idx=i) for fn, i in long]
    m.max_lt_idx = max_lt if max_lt is not None else max([i for _, i in long], default=-1)
    return m


def _names(frames):
    return [None if f is None else (f"LT{f.long_term_idx}" if f.long_term_idx is not None else f.frame_num)
            for f in frames]


def _state(m):
    return sorted(f.frame_num for f in m.short), sorted(f.long_term_idx for f in m.long)


def test_initial_list_mixed_short_and_long_term():
    # 8.2.4.2.1: short-term by descending PicNum (5 -> 7, 6, 4 ... here 7, 6, 4), then long-term
    # by ascending LongTermPicNum, whatever order they were stored in
    m = _dpb(short=[4, 7, 6], long=[(2, 3), (1, 0)])
    assert _names(m.initial_list(8, MAXFN)) == [7, 6, 4, "LT0", "LT3"]
    # cut to num_ref_idx_active; a list shorter than that is padded with "no reference picture"
    assert _names(m.build_list(8, MAXFN, 2)) == [7, 6]
    assert _names(_dpb(short=[7]).build_list(8, MAXFN, 2)) == [7, None]


def test_pic_num_across_frame_num_wrap():
    # 8.2.4.1 (8-27): frame_num 14, 15 seen from frame_num 1 have FrameNumWrap -2, -1; 0 stays 0
    m = _dpb(short=[14, 15, 0])
    assert [m.pic_num(f, 1, MAXFN) for f in m.short] == [-2, -1, 0]
    assert _names(m.initial_list(1, MAXFN)) == [0, 15, 14]
    # list modification across the wrap (8-34, 8-36): CurrPicNum 1, abs_diff 3 -> picNumNoWrap
    # 1 - 3 + 16 = 14 > CurrPicNum -> picNum 14 - 16 = -2, the frame with frame_num 14
    assert _names(m.build_list(1, MAXFN, 3, [(0, 2)])) == [14, 0, 15]
    # idc 0, abs_diff 2: 1 - 2 + 16 = 15 -> picNum -1 (frame_num 15) and picNumL0Pred = 15; then
    # idc 1 adds (8-35), abs_diff 1: 15 + 1 = 16 >= MaxPicNum -> 0 <= CurrPicNum -> picNum 0
    assert _names(m.build_list(1, MAXFN, 3, [(0, 1), (1, 0)])) == [15, 0, 14]
    # idc 1, abs_diff 15 from pred 15: 30 - 16 = 14 > CurrPicNum -> picNum -2 (frame_num 14)
    assert _names(m.build_list(1, MAXFN, 3, [(0, 1), (1, 14)])) == [15, 14, 0]
    # MMCO 1 across the wrap: picNumX = CurrPicNum - (difference_of_pic_nums_minus1 + 1) = 1 - 3 = -2
    m.mark(RefFrame(1), False, MAXFN, 4, mmco=((1, 2),))
    assert _state(m) == ([0, 1, 15], [])


def test_rplm_previous_then_long_term():
    # the encoder's switch-back list: idc 0 / abs_diff_pic_num_minus1 0 (previous picture at
    # index 0), idc 2 / long_term_pic_num 1 (at index 1); initial list [9, 8, LT0, LT1]
    m = _dpb(short=[8, 9], long=[(3, 0), (5, 1)])
    assert _names(m.build_list(10, MAXFN, 2, [(0, 0), (2, 1)])) == [9, "LT1"]
    # (8-37): the moved picture's later copy leaves, the others shift back
    assert _names(m.build_list(10, MAXFN, 4, [(2, 1)])) == ["LT1", 9, 8, "LT0"]
    assert _names(m.build_list(10, MAXFN, 4, [(0, 1)])) == [8, 9, "LT0", "LT1"]


def test_mmco3_into_free_and_occupied_index():
    # 8.2.5.4.3 after MMCO 4 opened indices 0..1: previous picture (PicNum 9 = 10 - 1) -> LT1 (free)
    m = _dpb(short=[9], long=[(3, 0)], max_lt=-1)
    m.mark(RefFrame(10), False, MAXFN, 3, mmco=((4, 2), (3, 0, 1)))
    assert _state(m) == ([10], [0, 1])
    assert [f.frame_num for f in m.long if f.long_term_idx == 1] == [9]
    # into the occupied index 0: the frame that held it (frame_num 3) becomes unused
    m.mark(RefFrame(11), False, MAXFN, 3, mmco=((4, 2), (3, 0, 0)))
    assert _state(m) == ([11], [0, 1])
    assert [f.frame_num for f in m.long if f.long_term_idx == 0] == [10]
    # an index beyond MaxLongTermFrameIdx is not allowed
    with pytest.raises(BitstreamError):
        _dpb(short=[9], max_lt=0).mark(RefFrame(10), False, MAXFN, 3, mmco=((3, 0, 1),))


def test_mmco1_drops_the_oldest_short_term_picture():
    # DPB [5, 6, 7] + LT0 with max_num_ref_frames 4 is full; storing 7 into the free index 1
    # would leave 5, 6, 8, LT0, LT1 = 5 frames, so 5 goes first: difference_of_pic_nums_minus1 =
    # CurrPicNum - picNumX - 1 = 8 - 5 - 1 = 2
    m = _dpb(short=[5, 6, 7], long=[(1, 0)], max_lt=1)
    m.mark(RefFrame(8), False, MAXFN, 4, mmco=((4, 2), (1, 2), (3, 0, 1)))
    assert _state(m) == ([6, 8], [0, 1])


def test_mmco4_shrinks_the_index_range_and_mmco2_and_6():
    # 8.2.5.4.4: max_long_term_frame_idx_plus1 = 1 keeps only index 0; = 0 keeps none
    m = _dpb(short=[4], long=[(1, 0), (2, 1), (3, 2)])
    m.mark(RefFrame(5), False, MAXFN, 5, mmco=((4, 1),))
    assert _state(m) == ([4, 5], [0]) and m.max_lt_idx == 0
    m.mark(RefFrame(6), False, MAXFN, 5, mmco=((4, 0),))
    assert _state(m) == ([4, 5, 6], []) and m.max_lt_idx == -1
    # MMCO 2 (long-term picture unused) and MMCO 6 (the current picture becomes long-term)
    m = _dpb(short=[4], long=[(1, 0), (2, 1)])
    m.mark(RefFrame(5), False, MAXFN, 4, mmco=((2, 0), (6, 0)))
    assert _state(m) == ([4], [0, 1])
    assert [f.frame_num for f in m.long if f.long_term_idx == 0] == [5]
    with pytest.raises(NotImplementedError):
        m.mark(RefFrame(6), False, MAXFN, 4, mmco=((5,),))


def test_sliding_window_only_without_mmco_and_idr():
    # 8.2.5.3: numShortTerm + numLongTerm == Max(max_num_ref_frames, 1) -> the short-term frame
    # with the smallest FrameNumWrap leaves (15 seen from 1 wraps to -1)
    m = _dpb(short=[15, 0], long=[(7, 0)])
    m.mark(RefFrame(1), False, MAXFN, 3)
    assert _state(m) == ([0, 1], [0])
    # an IDR empties both sets; long_term_reference_flag makes it LT0
    m.mark(RefFrame(0), True, MAXFN, 3)
    assert _state(m) == ([0], []) and m.max_lt_idx == -1
    m.mark(RefFrame(0), True, MAXFN, 3, long_term_reference_flag=True)
    assert _state(m) == ([], [0]) and m.max_lt_idx == 0


def test_error_missing_picture():
    m = _dpb(short=[8, 9], long=[(3, 0)], max_lt=1)
    with pytest.raises(BitstreamError):   # no short-term frame with PicNum 10 - 3 = 7
        m.mark(RefFrame(10), False, MAXFN, 4, mmco=((1, 2),))
    with pytest.raises(BitstreamError):
        m.mark(RefFrame(10), False, MAXFN, 4, mmco=((3, 4, 1),))
    with pytest.raises(BitstreamError):   # no long-term frame with LongTermPicNum 1
        m.mark(RefFrame(10), False, MAXFN, 4, mmco=((2, 1),))
    with pytest.raises(BitstreamError):
        m.build_list(10, MAXFN, 2, [(0, 0), (2, 1)])
    with pytest.raises(BitstreamError):   # PicNum 10 - 3 = 7 is not in the DPB
        m.build_list(10, MAXFN, 2, [(0, 2)])


def test_error_dpb_over_bound():
    # MMCO 3 into a free index without dropping a short-term frame: 8, 10, LT0, LT1 with
    # max_num_ref_frames 3 (the case the encoder's marking model has to avoid with MMCO 1)
    m = _dpb(short=[8, 9], long=[(3, 0)], max_lt=1)
    with pytest.raises(BitstreamError, match="DPB"):
        m.mark(RefFrame(10), False, MAXFN, 3, mmco=((4, 2), (3, 0, 1)))
    # max_num_ref_frames 0 counts as 1
    m = _dpb(short=[8])
    m.mark(RefFrame(9), False, MAXFN, 0)
    assert _state(m) == ([9], [])


# ---- the same rules through the slice header parser -------------------------------------------

class _W:
    def __init__(self):
        self.bits = []

    def u(self, v, n):
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def ue(self, v):
        v += 1
        n = v.bit_length()
        self.u(0, n - 1)
        self.u(v, n)

    def se(self, v):
        self.ue(2 * v - 1 if v > 0 else -2 * v)

    def nal(self, hdr):
        b = self.bits + [1]
        b += [0] * (-len(b) % 8)
        body = bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))
        return bytes([hdr]) + body


def _slice(first_mb, slice_type, frame_num, idr=False, mmco=None):
    """Slice header (7.3.3) up to dec_ref_pic_marking() for the test PPS below; the caller appends
    slice_qp_delta. Only the header parsing and the picture bookkeeping are exercised."""
    w = _W()
    w.ue(first_mb)
    w.ue(slice_type)
    w.ue(0)
    w.u(frame_num, 4)
    if idr:
        w.ue(0)
    if slice_type == 0:
        w.u(0, 1)   # num_ref_idx_active_override_flag
        w.u(0, 1)   # ref_pic_list_modification_flag_l0
    if idr:
        w.u(0, 2)
    elif mmco is None:
        w.u(0, 1)
    else:
        w.u(1, 1)
        for op in mmco:
            for v in op:
                w.ue(v)
        w.ue(0)
    return w


def test_error_slices_disagree_on_marking(monkeypatch):
    """Two slices of one picture (same frame_num, first_mb 1 after 0) must carry the same
    dec_ref_pic_marking() (7.4.3.3)."""
    d = D.H264Decoder()
    d.sps[0] = D.SPS(66, 0xC0, 10, 4, 2, 0, 3, 2, 1, (0, 0, 0, 0))   # log2_max_frame_num 4, 3 reference frames, 2 x 1 MBs
    d.pps[0] = D.PPS(sps_id=0, entropy_coding_mode=0, num_ref_idx_l0=1, pic_init_qp=26, chroma_qp_index_offset=0,
                     deblocking_filter_control_present=0, constrained_intra_pred=0, redundant_pic_cnt_present=0)
    monkeypatch.setattr(d, "_slice_data", lambda *a, **k: None)   # headers only
    monkeypatch.setattr(d, "_deblock_picture", lambda: None)

    def feed(w, idr=False):
        w.se(0)   # slice_qp_delta
        d.decode_nal(w.nal(0x65 if idr else 0x41))

    feed(_slice(0, 2, 0, idr=True), idr=True)
    feed(_slice(0, 0, 1))
    feed(_slice(0, 0, 2, mmco=((4, 1), (3, 0, 0))))
    with pytest.raises(BitstreamError, match="disagree"):
        feed(_slice(1, 0, 2))                       # second slice of picture 2 without the MMCOs
    d.cur = None                                    # drop the broken picture
    feed(_slice(0, 0, 2, mmco=((4, 1), (3, 0, 0))))
    feed(_slice(1, 0, 2, mmco=((4, 1), (3, 0, 0))))   # agreeing slices are fine
    d.flush()
    assert _state(d.marking) == ([0, 2], [0])       # 1 -> LT0; 0 and 2 short-term (max_num_ref_frames 3)
