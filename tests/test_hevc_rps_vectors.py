"""Hand-worked vectors for the reference picture management the HEVC long-term reference cache
needs from the test decoder (models/hevc/decoder.py): picture order count (8.3.1), the long-term
part of the slice header's RPS (7.3.6.1), RPS derivation (8.3.2) and list 0 with modification
(7.3.6.2, 8.3.4), on hand-built decoded picture buffers. The expected values are worked from the
H.265 text, not from the encoders; no encoder runs here. The bit strings are written out below.
No independent HEVC decoder is available to these tests, so these vectors are what pins the rules
every encoder stream is then checked against (tests/test_hevc_ltr.py decodes the encoders'
packets, whose headers write_slice_header produced, through the same functions)."""
import pytest

from selkies_gstreamer_amd.models.hevc import decoder as D


def _bits(s: str) -> D.Bits:
    s = s.replace(" ", "")
    s += "0" * (-len(s) % 8)
    return D.Bits(bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8)))


def _u16(v: int) -> str:
    return format(v, "016b")


SPS = D.Sps(log2_poc_lsb=16, long_term=True, lt_ref_pics_sps=[], max_dec_pic_buffering_minus1=4)


def test_poc_across_an_lsb_wrap():
    # log2_max_pic_order_cnt_lsb 16: MaxLsb 65536, half 32768
    assert D.pic_order_cnt(65535, 65534, 0, 16) == (65535, 0)
    # lsb < prevLsb and prevLsb - lsb >= MaxLsb / 2: the MSB steps up
    assert D.pic_order_cnt(0, 65535, 0, 16) == (65536, 65536)
    assert D.pic_order_cnt(1, 0, 65536, 16) == (65537, 65536)
    # lsb > prevLsb and lsb - prevLsb > MaxLsb / 2: a picture from before the wrap, the MSB steps down
    assert D.pic_order_cnt(65534, 2, 65536, 16) == (65534, 0)
    # exactly half apart: forward stays in the cycle (not > half), backward wraps (>= half)
    assert D.pic_order_cnt(32768, 0, 0, 16) == (32768, 0)
    assert D.pic_order_cnt(0, 32768, 0, 16) == (65536, 65536)
    # a small LSB (4 bits) wraps every 16 pictures
    poc, lsb, msb = [], 14, 0
    for nxt in (15, 0, 1):
        p, msb = D.pic_order_cnt(nxt, lsb, msb, 4)
        lsb = nxt
        poc.append(p)
    assert poc == [15, 16, 17]


def test_long_term_syntax_of_the_slice_header():
    # num_long_term_pics ue(v): 0 -> "1"
    assert D.parse_lt_rps(_bits("1"), SPS, 0) == []
    # one entry: ue(1) = "010", poc_lsb_lt u(16) = 9, used_by_curr_pic_lt_flag 1, delta_poc_msb_present_flag 0
    b = _bits("010" + _u16(9) + "1" + "0")
    assert D.parse_lt_rps(b, SPS, 0) == [(9, 1, 0, 0)] and b.p == 3 + 16 + 2
    # three entries: ue(3) = "00100"; the third carries an MSB (delta_poc_msb_cycle_lt ue(1) = "010")
    b = _bits("00100" + _u16(9) + "10" + _u16(65535) + "10" + _u16(40) + "01" + "010")
    assert D.parse_lt_rps(b, SPS, 0) == [(9, 1, 0, 0), (65535, 1, 0, 0), (40, 0, 1, 1)]
    assert b.p == 5 + 3 * 18 + 3


def test_rps_one_short_term_and_long_term_entries():
    st = [(-1, 1)]   # the SPS's one short-term RPS: the previous picture, used
    # 0 long-term entries
    r = D.derive_rps(20, st, [], [(19, False)], 16)
    assert r == {"st_curr_before": [19], "st_curr_after": [], "st_foll": [], "lt_curr": [], "lt_foll": []}
    # 1 long-term entry, by LSB
    r = D.derive_rps(20, st, [(9, 1, 0, 0)], [(9, True), (19, False)], 16)
    assert r["st_curr_before"] == [19] and r["lt_curr"] == [9] and r["lt_foll"] == []
    # 3 long-term entries in header order; one is kept but not used by the current picture
    dpb = [(9, True), (12, True), (15, True), (19, False)]
    r = D.derive_rps(20, st, [(9, 1, 0, 0), (12, 0, 0, 0), (15, 1, 0, 0)], dpb, 16)
    assert r["lt_curr"] == [9, 15] and r["lt_foll"] == [12] and r["st_curr_before"] == [19]
    # after a wrap of the LSBs: picture 65530 is named by its LSB from picture 65540 (LSB 4)
    r = D.derive_rps(65540, st, [(65530, 1, 0, 0)], [(65530, True), (65539, False)], 16)
    assert r["lt_curr"] == [65530] and r["st_curr_before"] == [65539]
    # with an MSB: POC = 65540 - 1 * 65536 - (4 - 2) = 2
    r = D.derive_rps(65540, st, [(2, 1, 1, 1)], [(2, True), (65538, True), (65539, False)], 16)
    assert r["lt_curr"] == [2]


def test_short_term_picture_turns_long_term_in_the_next_picture():
    st = [(-1, 1)]
    # picture 10: its short-term reference is 9
    r = D.derive_rps(10, st, [], [(9, False)], 16)
    assert r["st_curr_before"] == [9]
    # picture 11: 10 is the short-term reference, 9 (still short-term in the DPB) is named long-term
    r = D.derive_rps(11, st, [(9, 1, 0, 0)], [(9, False), (10, False)], 16)
    assert r["st_curr_before"] == [10] and r["lt_curr"] == [9]
    # once long-term, a short-term entry cannot name it
    with pytest.raises(D.BitstreamError):
        D.derive_rps(11, [(-2, 1)], [(9, 1, 0, 0)], [(9, False), (10, False)], 16)
    # through the decoder's bookkeeping: the DPB marks it and drops what the RPS does not name
    dec = D.HevcDecoder()
    dec.sps = SPS
    dec.dpb = [{"poc": p, "lt": False, "planes": None} for p in (8, 9, 10)]
    dec.prev_lsb, dec.prev_msb = 10, 0
    dec.cur = {}
    dec._reference_pictures(True, False, (11, ((-1, 1),), ((9, 1, 0, 0),)))
    assert dec.poc == 11 and [(d["poc"], d["lt"]) for d in dec.dpb] == [(9, True), (10, False)]


def test_list0_without_and_with_modification():
    rps = {"st_curr_before": [19], "st_curr_after": [], "st_foll": [], "lt_curr": [9], "lt_foll": [12]}
    # NumPicTotalCurr 2: entries are 1 bit. flag 0 -> the short-term picture first
    assert D.parse_list_modification(_bits("0"), 2, 1) is None
    assert D.build_list0(rps, 1, None) == [19]
    # flag 1, list_entry_l0[0] = 1 ("1"): the long-term picture
    b = _bits("1" + "1")
    e = D.parse_list_modification(b, 2, 1)
    assert e == [1] and b.p == 2 and D.build_list0(rps, 1, e) == [9]
    # NumPicTotalCurr 3: 2 bits. entry 2 ("10") = the second long-term picture
    rps3 = dict(rps, lt_curr=[9, 15])
    b = _bits("1" + "10")
    e = D.parse_list_modification(b, 3, 1)
    assert e == [2] and b.p == 3 and D.build_list0(rps3, 1, e) == [15]
    # NumPicTotalCurr 9 (eight long-term pictures): 4 bits. entry 8 ("1000") = the last of them
    rps9 = dict(rps, lt_curr=[1, 2, 3, 4, 5, 6, 7, 8])
    b = _bits("1" + "1000")
    e = D.parse_list_modification(b, 9, 1)
    assert e == [8] and b.p == 5 and D.build_list0(rps9, 1, e) == [8]
    b = _bits("1" + "0011")
    assert D.build_list0(rps9, 1, D.parse_list_modification(b, 9, 1)) == [3]
    # NumPicTotalCurr 1: no syntax at all
    b = _bits("1")
    assert D.parse_list_modification(b, 1, 1) is None and b.p == 0
    # without modification a longer list repeats the pictures in order (8-8)
    assert D.build_list0(rps3, 4, None) == [19, 9, 15, 19]


def test_rps_entry_names_a_missing_picture():
    with pytest.raises(D.BitstreamError, match="long-term"):
        D.derive_rps(20, [(-1, 1)], [(7, 1, 0, 0)], [(9, True), (19, False)], 16)
    with pytest.raises(D.BitstreamError, match="short-term"):
        D.derive_rps(20, [(-1, 1)], [], [(9, True), (18, False)], 16)


def test_list_entry_out_of_range():
    rps = {"st_curr_before": [19], "st_curr_after": [], "st_foll": [], "lt_curr": [9, 15], "lt_foll": []}
    # 2 bits can say 3, NumPicTotalCurr is 3
    e = D.parse_list_modification(_bits("1" + "11"), 3, 1)
    with pytest.raises(D.BitstreamError, match="list_entry_l0"):
        D.build_list0(rps, 1, e)


def _decoder_at_picture_20(max_dec):
    dec = D.HevcDecoder()
    dec.sps = D.Sps(log2_poc_lsb=16, long_term=True, lt_ref_pics_sps=[], max_dec_pic_buffering_minus1=max_dec)
    dec.dpb = [{"poc": 9, "lt": True, "planes": None}, {"poc": 12, "lt": True, "planes": None},
               {"poc": 19, "lt": False, "planes": None}]
    dec.prev_lsb, dec.prev_msb = 19, 0
    dec.cur = {}
    return dec


def test_slices_of_a_picture_disagree_on_their_rps():
    dec = _decoder_at_picture_20(3)
    key = (20, ((-1, 1),), ((9, 1, 0, 0), (12, 1, 0, 0)))
    dec._reference_pictures(True, False, key)
    dec._reference_pictures(False, False, key)            # the same syntax: fine
    with pytest.raises(D.BitstreamError, match="disagree"):
        dec._reference_pictures(False, False, (20, ((-1, 1),), ((9, 1, 0, 0),)))


def test_rps_larger_than_the_dpb():
    key = (20, ((-1, 1),), ((9, 1, 0, 0), (12, 1, 0, 0)))
    _decoder_at_picture_20(3)._reference_pictures(True, False, key)    # 3 pictures, sps_max_dec_pic_buffering_minus1 3
    with pytest.raises(D.BitstreamError, match="sps_max_dec_pic_buffering_minus1"):
        _decoder_at_picture_20(2)._reference_pictures(True, False, key)
