"""debug_buffer names of the HIP back end after its split into a codec-neutral session and one
tail per codec (csrc/runtime/hip_session.h, *_tail.h): every name the CPU back end of a codec
answers is answered by the HIP one with the same byte count, the names of another codec's buffers
are unknown to both ("mbs" on HEVC and AV1, AV1's "coefs"), and an encoder closed with a frame
in flight drains its stream before the tail's buffers are freed."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import Av1Encoder, H264Encoder, HevcEncoder, hip_device_count
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop

pytestmark = pytest.mark.gpu

W = H = 128
ENCODERS = dict(h264=H264Encoder, hevc=HevcEncoder, av1=Av1Encoder)
# the front end's names both back ends share; the long-term cache is on (one slot) so that its names exist
FRONT = ("src_y", "src_u", "src_v", "ref_y", "ref_u", "ref_v", "me", "tasks", "ltr_state", "ltr_task", "ltr0_y")
# codec_debug of the CPU back end (sk_api.cpp) without the cache's names, which are in FRONT, and
# without HEVC's "pc_dbg": the CPU encoder's own trace of its parallel CABAC pass, which the HIP back
# end never had (HIP_ONLY below holds its counterparts), and without HEVC's "bins": the binariser's
# entries with their context indices, which k_pc_model replaces by modelled states on the device
CODEC = dict(h264=("ref1_y", "mbs", "coefs", "mb_dirty", "aq", "fs_mv"),
             hevc=("cus", "sao", "coefs", "bin_n"),
             av1=("blk", "levels", "av1_geo", "av1_qidx"))
# intermediate buffers of the HIP coding kernels that the CPU encoders do not have
HIP_ONLY = dict(h264=(),
                hevc=("cu_t", "cu_r", "tail", "sub", "sub_size", "row_bits"),
                av1=("tok_n", "tokc", "tile_ntok", "frame", "tile_size"))
# another codec's buffers: unknown to both back ends
FOREIGN = dict(h264=("cus", "blk", "levels"), hevc=("mbs", "blk", "levels"), av1=("mbs", "coefs", "cus"))


def _encoder(codec, backend):
    # adaptive QP on: the CPU back end holds "aq" only then
    return ENCODERS[codec](W, H, stripe_height=64, backend=backend, ltr_slots=1, aq_strength=1.0)


def _nbytes(enc, name):
    try:
        return enc.debug_buffer(name).nbytes
    except KeyError:
        return None


@pytest.mark.parametrize("codec", list(ENCODERS))
def test_hip_debug_names(codec):
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    src = SyntheticDesktop(W, H, kind="motion")
    frames = [src.frame(t) for t in range(3)]
    cpu, gpu = _encoder(codec, "cpu"), _encoder(codec, "hip")
    for t in range(2):   # key + inter
        pc, pg = cpu.encode(frames[t], t), gpu.encode(frames[t], t)
        assert [p.data for p in pg] == [p.data for p in pc], f"frame {t}: packets differ"
    for name in FRONT + CODEC[codec]:
        nc, ng = _nbytes(cpu, name), _nbytes(gpu, name)
        print(f"{codec} {name}: cpu {nc} hip {ng}")
        assert nc is not None and nc > 0 and ng == nc, f"{name}: cpu {nc} bytes, hip {ng}"
    for name in HIP_ONLY[codec]:
        assert _nbytes(cpu, name) is None and (_nbytes(gpu, name) or 0) > 0, name
    for name in FOREIGN[codec]:
        for enc in (cpu, gpu):
            with pytest.raises(KeyError):
                enc.debug_buffer(name)
    # a second HIP encoder destroyed with a launched frame that was never finished
    other = _encoder(codec, "hip")
    other.upload(frames[0], 0)
    other.launch()
    other.close()
    # the device and the first encoder are as before
    pc, pg = cpu.encode(frames[2], 2), gpu.encode(frames[2], 2)
    assert [p.data for p in pg] == [p.data for p in pc], "frame 2: packets differ"
    gpu.close()
    cpu.close()
