"""CPU: the channeliser's demodulators, power squelch and gate (rxgpu_chan_params.mode .. squelch_zero) -- argument checks without a device,
the C layout of the parameters, and the reference chain the GPU tests hold the device to (tests/chan_modes_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rx_tools_amd as R
from chan_modes_ref import burst_capture, chan_modes_stream, demod_thread_gate
from support import ROOT, have_ref, ref_chan_stream, sig_fm, sig_noise

skip_without_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built (needs the reference checkout)")
RXGPU_EINVAL = -2


@pytest.mark.parametrize("field,value", [("mode", 5), ("mode", -1), ("squelch_level", -1), ("conseq_squelch", -3), ("squelch_zero", 2),
                                         ("squelch_zero", -1)])
def test_create_refuses_invalid_new_fields(field, value):
    """refused with RXGPU_EINVAL naming the field, before the device is touched (without a GPU the valid parameters fail on the device instead)"""
    L = R.lib()
    p = R.ChanParams(10, 0, 4, 1)
    setattr(p, field, value)
    h = C.c_void_p()
    sw = R.sine_table(10)
    assert L.rxgpu_chan_create(C.byref(h), C.byref(p), 1, 2 * 1024, sw.ctypes.data) == RXGPU_EINVAL
    assert field.encode() in L.rxgpu_last_error()
    import torch
    if not torch.cuda.is_available():
        setattr(p, field, 0)
        rc = L.rxgpu_chan_create(C.byref(h), C.byref(p), 1, 2 * 1024, sw.ctypes.data)
        assert rc != RXGPU_EINVAL and b"no HIP device" in L.rxgpu_last_error()


def test_chan_params_layout_matches_header(tmp_path):
    """ctypes ChanParams == struct rxgpu_chan_params as the host C compiler lays it out from include/rxgpu.h"""
    names = [f[0] for f in R.ChanParams._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rxgpu.h"\nint main(void){printf("%zu", sizeof(rxgpu_chan_params));' +
                   "".join('printf(" %%zu", offsetof(rxgpu_chan_params, %s));' % n for n in names) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(R.ChanParams)
    assert got[1:] == [getattr(R.ChanParams, n).offset for n in names]
    assert names[-5:] == ["mode", "output_scale", "squelch_level", "conseq_squelch", "squelch_zero"]
    assert (R.RXGPU_MODE_FM, R.RXGPU_MODE_AM, R.RXGPU_MODE_USB, R.RXGPU_MODE_LSB, R.RXGPU_MODE_RAW) == (0, 1, 2, 3, 4)


def test_positional_params_keep_todays_meaning():
    """bench.py and the existing tests build ChanParams with up to nine positional fields: the new ones are then 0 (FM, no squelch)"""
    p = R.ChanParams(10, 384, 256, 1, 1, 7, 19531, 8000, 0)
    assert (p.mode, p.output_scale, p.squelch_level, p.conseq_squelch, p.squelch_zero) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("conseq,zero,want_gate", [
    (0, 0, [1, 0] + [1] * 12 + [0]),
    (0, 1, [2, 0] + [2] * 12 + [0]),
    (10, 0, [1, 0] + [0] * 10 + [1, 1, 0]),
    (10, 1, [2, 0] + [0] * 10 + [2, 2, 0]),
])
def test_gate_on_crafted_blocks(conseq, zero, want_gate):
    """silent, loud, silent x 12, loud: the count starts at 11 (demod_init), a loud block resets it, the hair trigger clamps it at conseq + 1"""
    bin_e, wpb, n_ch = 6, 8, 4
    block_len = 2 * (wpb << bin_e)
    loud = sig_noise(block_len, seed=5, amp=3000)
    pattern = [0, 1] + [0] * 12 + [1]
    iq = np.concatenate([loud if p else np.zeros(block_len, np.int16) for p in pattern])
    backends = ["oracle"] + (["ref"] if have_ref() else [])
    for backend in backends:
        r = chan_modes_stream(iq, block_len, bin_e, 3, n_ch, mode=R.RXGPU_MODE_AM, squelch_level=20, conseq_squelch=conseq, squelch_zero=zero,
                              backend=backend)
        for c in range(n_ch):
            assert r["gate"][c].tolist() == want_gate, backend
            assert np.all(r["sr"][c, np.array(pattern) == 0] == 0) and np.all(r["sr"][c, np.array(pattern) == 1] >= 20)
        assert np.all(r["hits"] == 0)
        for b, g in enumerate(want_gate):
            if g == 2:
                assert not r["out"][:, b * wpb:(b + 1) * wpb].any()
    # the rule itself, from the default count: the first quiet block after demod_init is already past -t 10
    assert demod_thread_gate(12, 5, 10, 0) == (11, 1) and demod_thread_gate(12, 5, 10, 1) == (12, 2) and demod_thread_gate(12, 0, 10, 0) == (12, 0)


@pytest.mark.ref
@skip_without_ref
@pytest.mark.parametrize("bin_e,first_bin,n_channels,block_len,n_blocks", [(10, 900, 64, 2 * 8192, 3), (5, 3, 20, 2 * 1024, 3), (12, 100, 7, 2 * 8192, 4)])
@pytest.mark.parametrize("custom_atan", [1, 0])
def test_helper_fm_equals_ref_chan_stream(bin_e, first_bin, n_channels, block_len, n_blocks, custom_atan):
    """mode FM, squelch off: both backends of the new helper == support.ref_chan_stream (the existing reference-built channeliser checker)"""
    for iq in (sig_fm(n_blocks * block_len // 2, seed=70, amp=9000), sig_noise(n_blocks * block_len, seed=71)):
        want, want_pre, _ = ref_chan_stream(iq, block_len, bin_e, first_bin, n_channels, custom_atan)
        for backend in ("ref", "oracle"):
            r = chan_modes_stream(iq, block_len, bin_e, first_bin, n_channels, custom_atan, backend=backend)
            assert np.array_equal(r["out"], want) and np.array_equal(r["pre"], want_pre), backend
            assert np.all(r["hits"] == 11) and not r["gate"].any() and not r["sr"].any()


@pytest.mark.ref
@skip_without_ref
@pytest.mark.parametrize("mode,scale,level,conseq,zero,audio,nco", [
    (1, 3, 0, 0, 0, False, 0), (2, 3, 0, 0, 0, False, 0), (3, 1, 0, 0, 0, False, 0), (4, 1, 0, 0, 0, False, 0),
    (0, 1, 1, 2, 0, False, 0), (1, 1, 1, 0, 1, True, 0), (0, 1, 1, 10, 1, True, 0), (1, 1, 1, 0, 1, False, 1),
])
def test_helper_oracle_backend_equals_ref_backend(mode, scale, level, conseq, zero, audio, nco):
    """the restatement backend (what the GPU tests use) == the reference-built one on every mode, the squelch, the gate and the audio stages"""
    bin_e, first_bin, n_ch, block_len, n_blocks = (8, 0, 64, 2 * 4096, 12) if nco else (7, 0, 128, 2 * 4096, 12)
    iq, split = burst_capture(n_blocks, block_len, bin_e, first_bin, n_ch, seed=8, nco=nco)
    if level:
        level = split
    kw = dict(custom_atan=0, mode=mode, output_scale=scale, squelch_level=level, conseq_squelch=conseq, squelch_zero=zero, nco=nco)
    if audio:
        kw.update(deemph=1, a=7, rate_out=19531, rate_out2=8000)
    a = chan_modes_stream(iq, block_len, bin_e, first_bin, n_ch, backend="ref", **kw)
    b = chan_modes_stream(iq, block_len, bin_e, first_bin, n_ch, backend="oracle", **kw)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    if level:
        assert a["gate"].any() and not a["gate"].all()
