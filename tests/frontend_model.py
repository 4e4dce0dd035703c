"""An independent model of the encoders' front end, numpy only: what every codec sees before it
codes anything. Nothing here is shared with csrc/; tests/test_frontend.py compares both back ends
with it.

  bt709_float     Y'CbCr of the BT.709 definition in float64, unrounded
  planes_int      the integer front end: resample, overlay composite, conversion, edge padding
  planes_planar   planar 4:2:0 input, padded
  damage          per-macroblock change flags between two sets of padded planes
  colour_signal   the colour description a stream announces, read from its sequence header

The integer coefficients are BT.709's, scaled by 256 (1024 for the chroma of a 2x2 quad sum) and
rounded; where plain rounding would leave a row sum off its target (220 or 256 for luma, zero for
chroma), the coefficient with the largest rounding error gives way, so that greys have no colour
and white reaches its rail. tests/test_frontend.py holds them to bt709_float."""
from __future__ import annotations

import numpy as np

KR, KB = 0.2126, 0.0722
KG = 1.0 - KR - KB

#                     R     G    B
_Y = {False: (47, 157, 16), True: (54, 183, 19)}
_CB = {False: (-26, -86, 112), True: (-29, -99, 128)}
_CR = {False: (112, -102, -10), True: (128, -116, -12)}


# ---- resampling and overlays ---------------------------------------------------------------------
def np_scale(src: np.ndarray, dw: int, dh: int) -> np.ndarray:
    sh, sw = src.shape[:2]
    stx, sty = (sw << 16) // dw, (sh << 16) // dh

    def pos(d, step):
        p = (((2 * d + 1).astype(np.int64) * step) >> 1) - 0x8000
        return np.maximum(p, 0)
    px, py = pos(np.arange(dw), stx), pos(np.arange(dh), sty)
    x0 = np.minimum(px >> 16, sw - 1)
    y0 = np.minimum(py >> 16, sh - 1)
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    wx, wy = ((px >> 8) & 255)[None, :, None], ((py >> 8) & 255)[:, None, None]
    s = src.astype(np.int64)

    def lerp(a, b, w):
        return (a * (256 - w) + b * w + 128) >> 8
    top = lerp(s[y0][:, x0], s[y0][:, x1], wx)
    bot = lerp(s[y1][:, x0], s[y1][:, x1], wx)
    return lerp(top, bot, wy).astype(np.uint8)


def composite(frame, img, x, y, tile=None):
    out = frame.copy()
    H, W = frame.shape[:2]
    h, w = img.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = xs - x, ys - y
    ok = (dx >= 0) & (dy >= 0)
    if tile:
        dx, dy = dx % tile[0], dy % tile[1]
    ok &= (dx < w) & (dy < h)
    src = img[np.clip(dy, 0, h - 1), np.clip(dx, 0, w - 1)].astype(np.uint32)
    a = src[..., 3:4]
    d = out[..., :3].astype(np.uint32)
    blended = ((src[..., :3] + (d * (255 - a) + 127) // 255) & 255).astype(np.uint8)
    m = ok & (a[..., 0] > 0)
    out[..., :3][m] = blended[m]
    return out


# ---- colour --------------------------------------------------------------------------------------
def _clamp_pad(a: np.ndarray, ph: int, pw: int) -> np.ndarray:
    """`a` grown to ph x pw: sample (y, x) of the result is a[min(y, h - 1), min(x, w - 1)]."""
    h, w = a.shape[:2]
    return a[np.minimum(np.arange(ph), h - 1)][:, np.minimum(np.arange(pw), w - 1)]


def bt709_float(bgrx: np.ndarray, full_range: bool):
    """(Y, Cb, Cr) in float64, unrounded and unclipped, of a BGRx picture (h, w, 4) by the BT.709
    definition: E'Y = Kr R + Kg G + Kb B, E'Cb = (B - E'Y) / (2 (1 - Kb)), E'Cr = (R - E'Y) /
    (2 (1 - Kr)) on R, G, B in 0..1, then Y = 16 + 219 E'Y, C = 128 + 224 E'C (limited range) or
    Y = 255 E'Y, C = 128 + 255 E'C (full range). Y has the picture's size; Cb and Cr are the mean
    over each 2x2 quad (an odd size repeats its last row / column)."""
    h, w = bgrx.shape[:2]
    p = _clamp_pad(bgrx, h + (h & 1), w + (w & 1)).astype(np.float64) / 255.0
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    ey = KR * r + KG * g + KB * b
    ecb = (b - ey) / (2.0 * (1.0 - KB))
    ecr = (r - ey) / (2.0 * (1.0 - KR))

    def quad_mean(a):
        return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4.0
    if full_range:
        return (255.0 * ey)[:h, :w], 128.0 + 255.0 * quad_mean(ecb), 128.0 + 255.0 * quad_mean(ecr)
    return (16.0 + 219.0 * ey)[:h, :w], 128.0 + 224.0 * quad_mean(ecb), 128.0 + 224.0 * quad_mean(ecr)


def convert_int(bgrx: np.ndarray, full_range: bool):
    """The integer conversion of a BGRx picture of even size: (Y, Cb, Cr) uint8, 4:2:0."""
    full_range = bool(full_range)
    b, g, r = (bgrx[..., i].astype(np.int32) for i in range(3))
    kr, kg, kb = _Y[full_range]
    y = (kr * r + kg * g + kb * b + 128) >> 8
    if not full_range:
        y = y + 16

    def quad_sum(a):
        return a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    rs, gs, bs = quad_sum(r), quad_sum(g), quad_sum(b)

    def chroma(k):
        return ((k[0] * rs + k[1] * gs + k[2] * bs + 512) >> 10) + 128
    return tuple(np.clip(a, 0, 255).astype(np.uint8) for a in (y, chroma(_CB[full_range]), chroma(_CR[full_range])))


def picture_bgrx(frame: np.ndarray, W: int, H: int, src_size=None, overlays=()) -> np.ndarray:
    """The W x H BGRx picture the conversion reads: the capture (its first src_size = (w, h)
    pixels, W x H without), resampled when the sizes differ, then the overlays (image, x, y, tile)
    in order, in picture coordinates."""
    sw, sh = src_size if src_size else (W, H)
    pic = np.ascontiguousarray(frame[:sh, :sw])
    if (sw, sh) != (W, H):
        pic = np_scale(pic, W, H)
    for img, x, y, tile in overlays:
        pic = composite(pic, img, x, y, tile)
    return pic


def padded_size(W: int, H: int):
    return (W + 15) // 16 * 16, (H + 15) // 16 * 16


def planes_int(frame: np.ndarray, W: int, H: int, full_range: bool, src_size=None, overlays=()):
    """The source planes of a W x H encoder for one captured BGRx frame, as the encoders lay them
    out: Y of whole macroblocks (both sizes rounded up to 16), Cb and Cr of half that size. A
    sample outside the picture is converted from the picture's pixels at the clamped coordinates
    (min(x, W - 1), min(y, H - 1)): the padding is done before the conversion, so a padding
    chroma sample is the quad of the clamped pixels, not a copy of the last chroma sample."""
    pw, ph = padded_size(W, H)
    return convert_int(_clamp_pad(picture_bgrx(frame, W, H, src_size, overlays), ph, pw), full_range)


def planes_unpadded(frame: np.ndarray, full_range: bool):
    """Y (h, w), Cb and Cr ((h + 1) / 2, (w + 1) / 2) of a BGRx picture of any size >= 1: the
    stand-alone converter's output (an odd size repeats its last row / column into the quad)."""
    h, w = frame.shape[:2]
    y, u, v = convert_int(_clamp_pad(frame, h + (h & 1), w + (w & 1)), full_range)
    return y[:h, :w], u, v


def planes_planar(fmt: str, planes, W: int, H: int):
    """The source planes for planar 4:2:0 input ("i420": (y, u, v); "nv12": (y, uv interleaved)):
    the samples themselves, each plane padded by repeating its last row and column."""
    if fmt.lower() == "nv12":
        y, uv = planes
        u, v = uv[:, 0::2], uv[:, 1::2]
    else:
        y, u, v = planes
    cw, ch = (W + 1) // 2, (H + 1) // 2
    assert y.shape == (H, W) and u.shape == (ch, cw) and v.shape == (ch, cw)
    pw, ph = padded_size(W, H)
    return _clamp_pad(y, ph, pw).copy(), _clamp_pad(u, ph // 2, pw // 2).copy(), _clamp_pad(v, ph // 2, pw // 2).copy()


def damage(prev_planes, planes, first: bool) -> np.ndarray:
    """(mb_h, mb_w) bool: the macroblocks in which any sample of the 16x16 luma area or of either
    8x8 chroma area differs between the two sets of padded planes; all of them on the first frame."""
    y, u, v = planes
    mb_h, mb_w = y.shape[0] // 16, y.shape[1] // 16
    if first:
        return np.ones((mb_h, mb_w), bool)
    out = np.zeros((mb_h, mb_w), bool)
    for a, b, n in zip(prev_planes, planes, (16, 8, 8)):
        out |= (a != b).reshape(mb_h, n, mb_w, n).any(axis=(1, 3))
    return out


# ---- colour signalling ---------------------------------------------------------------------------
class _Bits:
    """MSB-first bit reader."""

    def __init__(self, data: bytes):
        self.d, self.p = data, 0

    def u(self, n: int) -> int:
        v = 0
        for _ in range(n):
            if self.p >> 3 >= len(self.d):
                raise ValueError("read past the end of the header")
            v = (v << 1) | ((self.d[self.p >> 3] >> (7 - (self.p & 7))) & 1)
            self.p += 1
        return v

    def ue(self) -> int:
        z = 0
        while self.u(1) == 0:
            z += 1
            if z > 32:
                raise ValueError("bad ue(v)")
        return (1 << z) - 1 + (self.u(z) if z else 0)

    def se(self) -> int:
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)


def _nal_units(stream: bytes):
    """RBSPs of an Annex B byte stream: start codes removed, emulation prevention bytes dropped."""
    starts, i = [], 0
    while i + 2 < len(stream):
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            starts.append(i + 3)
            i += 3
        else:
            i += 1
    for k, s in enumerate(starts):
        e = starts[k + 1] - 3 if k + 1 < len(starts) else len(stream)
        out, zeros = bytearray(), 0
        for b in stream[s:e]:
            if zeros >= 2 and b == 3:
                zeros = 0
                continue
            out.append(b)
            zeros = zeros + 1 if b == 0 else 0
        yield bytes(out)


def _video_signal_type(b: _Bits):
    """video_signal_type and what precedes it in vui_parameters() (H.264 E.1.1 and HEVC E.2.1
    begin alike); the defaults of E.2.1 where a part is absent."""
    full, desc = 0, (2, 2, 2)
    if b.u(1):                      # aspect_ratio_info_present_flag
        if b.u(8) == 255:           # aspect_ratio_idc == Extended_SAR
            b.u(32)                 # sar_width, sar_height
    if b.u(1):                      # overscan_info_present_flag
        b.u(1)                      # overscan_appropriate_flag
    if b.u(1):                      # video_signal_type_present_flag
        b.u(3)                      # video_format
        full = b.u(1)               # video_full_range_flag
        if b.u(1):                  # colour_description_present_flag
            desc = (b.u(8), b.u(8), b.u(8))   # colour_primaries, transfer_characteristics, matrix_coefficients
    return (bool(full),) + desc


def _h264_sps(rbsp: bytes):
    """seq_parameter_set_data() of H.264 7.3.2.1.1 up to the colour description of its VUI (E.1.1)."""
    b = _Bits(rbsp)
    profile = b.u(8)
    b.u(16)                         # constraint_set flags, reserved_zero_2bits, level_idc
    b.ue()                          # seq_parameter_set_id
    if profile in (100, 110, 122, 244, 44, 83, 86, 118, 128, 138, 139, 134, 135):
        if b.ue() == 3:             # chroma_format_idc
            b.u(1)                  # separate_colour_plane_flag
        b.ue()                      # bit_depth_luma_minus8
        b.ue()                      # bit_depth_chroma_minus8
        b.u(1)                      # qpprime_y_zero_transform_bypass_flag
        if b.u(1):                  # seq_scaling_matrix_present_flag
            raise NotImplementedError("scaling matrices")
    b.ue()                          # log2_max_frame_num_minus4
    poc_type = b.ue()               # pic_order_cnt_type
    if poc_type == 0:
        b.ue()                      # log2_max_pic_order_cnt_lsb_minus4
    elif poc_type == 1:
        b.u(1)                      # delta_pic_order_always_zero_flag
        b.se()                      # offset_for_non_ref_pic
        b.se()                      # offset_for_top_to_bottom_field
        for _ in range(b.ue()):     # num_ref_frames_in_pic_order_cnt_cycle
            b.se()
    b.ue()                          # max_num_ref_frames
    b.u(1)                          # gaps_in_frame_num_value_allowed_flag
    b.ue()                          # pic_width_in_mbs_minus1
    b.ue()                          # pic_height_in_map_units_minus1
    if not b.u(1):                  # frame_mbs_only_flag
        b.u(1)                      # mb_adaptive_frame_field_flag
    b.u(1)                          # direct_8x8_inference_flag
    if b.u(1):                      # frame_cropping_flag
        for _ in range(4):
            b.ue()
    if not b.u(1):                  # vui_parameters_present_flag
        return (False, 2, 2, 2)
    return _video_signal_type(b)


def _hevc_sps(rbsp: bytes):
    """seq_parameter_set_rbsp() of HEVC 7.3.2.2 up to the colour description of its VUI (E.2.1)."""
    b = _Bits(rbsp)
    b.u(4)                          # sps_video_parameter_set_id
    sub = b.u(3)                    # sps_max_sub_layers_minus1
    b.u(1)                          # sps_temporal_id_nesting_flag
    b.u(8)                          # profile_tier_level (7.3.3): general_profile_space, tier, profile_idc
    b.u(32)                         # general_profile_compatibility_flag[32]
    b.u(4)                          # progressive, interlaced, non-packed, frame-only
    b.u(32)                         # 43 reserved bits and general_inbld_flag / reserved
    b.u(12)
    b.u(8)                          # general_level_idc
    present = [(b.u(1), b.u(1)) for _ in range(sub)]   # sub_layer_profile / level_present_flag
    if sub:
        b.u(2 * (8 - sub))          # reserved_zero_2bits
    for prof, lev in present:
        if prof:
            b.u(32), b.u(32), b.u(24)   # 88 bits of sub-layer profile
        if lev:
            b.u(8)
    b.ue()                          # sps_seq_parameter_set_id
    if b.ue() == 3:                 # chroma_format_idc
        b.u(1)                      # separate_colour_plane_flag
    b.ue()                          # pic_width_in_luma_samples
    b.ue()                          # pic_height_in_luma_samples
    if b.u(1):                      # conformance_window_flag
        for _ in range(4):
            b.ue()
    b.ue()                          # bit_depth_luma_minus8
    b.ue()                          # bit_depth_chroma_minus8
    poc_bits = b.ue() + 4           # log2_max_pic_order_cnt_lsb_minus4
    for _ in range(sub + 1 if b.u(1) else 1):   # sps_sub_layer_ordering_info_present_flag
        b.ue(), b.ue(), b.ue()      # max_dec_pic_buffering_minus1, max_num_reorder_pics, max_latency_increase_plus1
    for _ in range(6):              # coding / transform block size limits, transform hierarchy depths
        b.ue()
    if b.u(1) and b.u(1):           # scaling_list_enabled_flag, sps_scaling_list_data_present_flag
        raise NotImplementedError("scaling list data")
    b.u(2)                          # amp_enabled_flag, sample_adaptive_offset_enabled_flag
    if b.u(1):                      # pcm_enabled_flag
        b.u(8)                      # pcm sample bit depths
        b.ue(), b.ue()              # PCM coding block size limits
        b.u(1)                      # pcm_loop_filter_disabled_flag
    for i in range(b.ue()):         # num_short_term_ref_pic_sets: st_ref_pic_set(i), 7.3.7
        if i and b.u(1):            # inter_ref_pic_set_prediction_flag
            raise NotImplementedError("predicted reference picture sets")
        neg, pos = b.ue(), b.ue()   # num_negative_pics, num_positive_pics
        for _ in range(neg + pos):
            b.ue()                  # delta_poc_s0/s1_minus1
            b.u(1)                  # used_by_curr_pic_s0/s1_flag
    if b.u(1):                      # long_term_ref_pics_present_flag
        for _ in range(b.ue()):     # num_long_term_ref_pics_sps
            b.u(poc_bits)           # lt_ref_pic_poc_lsb_sps
            b.u(1)                  # used_by_curr_pic_lt_sps_flag
    b.u(2)                          # sps_temporal_mvp_enabled_flag, strong_intra_smoothing_enabled_flag
    if not b.u(1):                  # vui_parameters_present_flag
        return (False, 2, 2, 2)
    return _video_signal_type(b)


def _av1_sequence_header(b: _Bits):
    """sequence_header_obu() of AV1 5.5.1 with color_config() 5.5.2."""
    profile = b.u(3)                # seq_profile
    b.u(1)                          # still_picture
    reduced = b.u(1)                # reduced_still_picture_header
    if reduced:
        b.u(5)                      # seq_level_idx[0]
    else:
        model, delay_bits = 0, 0
        if b.u(1):                  # timing_info_present_flag
            b.u(32), b.u(32)        # num_units_in_display_tick, time_scale
            if b.u(1):              # equal_picture_interval
                z = 0               # num_ticks_per_picture_minus_1, uvlc()
                while b.u(1) == 0:
                    z += 1
                b.u(z)
            model = b.u(1)          # decoder_model_info_present_flag
            if model:
                delay_bits = b.u(5) + 1   # buffer_delay_length_minus_1
                b.u(32)             # num_units_in_decoding_tick
                b.u(10)             # buffer_removal_time_length_minus_1, frame_presentation_time_length_minus_1
        display = b.u(1)            # initial_display_delay_present_flag
        for _ in range(b.u(5) + 1):   # operating_points_cnt_minus_1
            b.u(12)                 # operating_point_idc
            if b.u(5) > 7:          # seq_level_idx
                b.u(1)              # seq_tier
            if model and b.u(1):    # decoder_model_present_for_this_op
                b.u(delay_bits), b.u(delay_bits), b.u(1)
            if display and b.u(1):  # initial_display_delay_present_for_this_op
                b.u(4)
    wbits, hbits = b.u(4) + 1, b.u(4) + 1   # frame_width_bits_minus_1, frame_height_bits_minus_1
    b.u(wbits), b.u(hbits)          # max_frame_width_minus_1, max_frame_height_minus_1
    if not reduced and b.u(1):      # frame_id_numbers_present_flag
        b.u(7)                      # delta_frame_id_length_minus_2, additional_frame_id_length_minus_1
    b.u(3)                          # use_128x128_superblock, enable_filter_intra, enable_intra_edge_filter
    if not reduced:
        b.u(4)                      # interintra compound, masked compound, warped motion, dual filter
        order_hint = b.u(1)         # enable_order_hint
        if order_hint:
            b.u(2)                  # enable_jnt_comp, enable_ref_frame_mvs
        force_sct = 2 if b.u(1) else b.u(1)   # seq_choose_screen_content_tools : seq_force_screen_content_tools
        if force_sct > 0 and not b.u(1):      # seq_choose_integer_mv
            b.u(1)                  # seq_force_integer_mv
        if order_hint:
            b.u(3)                  # order_hint_bits_minus_1
    b.u(3)                          # enable_superres, enable_cdef, enable_restoration
    high = b.u(1)                   # color_config(): high_bitdepth
    if profile == 2 and high:
        b.u(1)                      # twelve_bit
    mono = 0 if profile == 1 else b.u(1)   # mono_chrome
    desc = (b.u(8), b.u(8), b.u(8)) if b.u(1) else (2, 2, 2)   # color_description_present_flag
    if not mono and desc == (1, 13, 0):   # sRGB in the identity matrix: full range by definition
        return (True,) + desc
    return (bool(b.u(1)),) + desc   # color_range


def _av1_obus(tu: bytes):
    """(obu_type, payload) of every OBU of a temporal unit in the low-overhead format (5.3)."""
    i = 0
    while i < len(tu):
        head = tu[i]
        i += 1
        if head & 4:                # obu_extension_flag
            i += 1
        if not head & 2:            # obu_has_size_field
            yield (head >> 3) & 15, tu[i:]
            return
        size, shift = 0, 0
        while True:                 # leb128()
            byte = tu[i]
            i += 1
            size |= (byte & 127) << shift
            shift += 7
            if not byte & 128:
                break
        yield (head >> 3) & 15, tu[i:i + size]
        i += size


def colour_signal(codec: str, packet: bytes):
    """(full_range, colour primaries, transfer characteristics, matrix coefficients) that the
    sequence header in `packet` announces. `packet` is an encoder packet: the 10-byte stripe header,
    then Annex B NAL units (H.264, HEVC) or a temporal unit of OBUs (AV1). The readers follow the
    syntax tables of the standards (H.264 7.3.2.1.1 / E.1.1, HEVC 7.3.2.2 / E.2.1, AV1 5.5.1 /
    5.5.2), not the encoders' writers."""
    payload = bytes(packet[10:])
    if codec == "av1":
        for kind, body in _av1_obus(payload):
            if kind == 1:           # OBU_SEQUENCE_HEADER
                return _av1_sequence_header(_Bits(body))
    else:
        for rbsp in _nal_units(payload):
            if codec == "h264" and rbsp[0] & 31 == 7:
                return _h264_sps(rbsp[1:])
            if codec == "hevc" and (rbsp[0] >> 1) & 63 == 33:
                return _hevc_sps(rbsp[2:])
    raise ValueError(f"no {codec} sequence header in the packet")
