"""-m gpu: the channeliser's am / usb / lsb / raw demodulators, power squelch and demod-thread gate (rxgpu_chan_params.mode .. squelch_zero)
against the reference chain of tests/chan_modes_ref.py, bit for bit: rows, pre and audio carries, squelch_hits, sr and gate."""
import numpy as np
import pytest

import rx_tools_amd as R
from chan_modes_ref import burst_capture, chan_modes_stream
from support import have_ref, oracle_chan_stream, ref_chan_stream, sig_fm, sig_noise

pytestmark = pytest.mark.gpu


def gpu_modes(iq, block_len, prm, n_runs=1, hits=None, how="sync"):
    """runs of the channeliser over the capture: (rows, pre, audio, hits, sr, gate, host_fixups)"""
    from gpu_support import to_dev, torch_cuda
    torch = torch_cuda()
    n = 1 << prm.bin_e
    n_blocks = len(iq) // block_len
    wpb = block_len // 2 // n
    per = (n_blocks + n_runs - 1) // n_runs
    raw = prm.mode == R.RXGPU_MODE_RAW
    ch = R.Channeliser(prm, per, block_len, R.sine_table(prm.bin_e))
    if hits is not None:
        ch.set_squelch_carry(hits)
    d_iq = to_dev(iq)
    outs, srs, gates, fix, b = [], [], [], 0, 0
    lens = []
    while b < n_blocks:
        nb = min(per, n_blocks - b)
        stride = (2 if raw else 1) * nb * wpb
        d_out = torch.zeros((prm.n_channels, stride), dtype=torch.int16, device="cuda")
        if how == "async":
            ch.run_async(d_iq.data_ptr() + b * block_len * 2, nb, block_len, d_out.data_ptr(), stride)
            lens.append(stride)
        else:
            w = ch.run(d_iq.data_ptr() + b * block_len * 2, nb, block_len, d_out.data_ptr(), stride)
            lens.append(w)
            sr, gate = ch.squelch_report(nb)
            srs.append(sr)
            gates.append(gate)
            fix += ch.host_fixups
        outs.append(d_out)
        b += nb
    first = 0                                     # the first block the report covers
    if how == "async":
        assert ch.wait() == lens[-1]
        # the report is what the wait retired: the last two runs (the runs run_async retired on its own are not kept)
        first = min(max(0, n_runs - 2) * per, n_blocks)
        sr, gate = ch.squelch_report(n_blocks - first)
        with pytest.raises(R.RxGpuError):
            ch.squelch_report(n_blocks)
        srs, gates, fix = [sr], [gate], ch.host_fixups
    rows = np.concatenate([o[:, :w].cpu().numpy() for o, w in zip(outs, lens)], axis=1)
    res = (rows, ch.get_carry(), ch.get_audio_carry().reshape(prm.n_channels, 3), ch.get_squelch_carry(), np.concatenate(srs, axis=1),
           np.concatenate(gates, axis=1), fix, first)
    ch.close()
    return res


def check(got, want, what=""):
    rows, pre, audio, hits, sr, gate, _, first = got
    assert rows.shape == want["out"].shape, what
    bad = np.argwhere(rows != want["out"])
    assert bad.size == 0, "%s first mismatch at %s: got %d want %d (%d bad)" % (what, bad[0], rows[tuple(bad[0])], want["out"][tuple(bad[0])], len(bad))
    assert np.array_equal(pre, want["pre"]), what
    assert np.array_equal(audio, want["audio"]), what
    assert np.array_equal(hits, want["hits"]), what
    assert np.array_equal(sr, want["sr"][:, first:]), what
    assert np.array_equal(gate, want["gate"][:, first:]), what


def params(bin_e, first_bin, n_channels, custom_atan=1, deemph=0, a=0, rate_out=0, rate_out2=-1, nco=0, mode=0, output_scale=0, level=0,
           conseq=0, zero=0):
    return R.ChanParams(bin_e, first_bin, n_channels, custom_atan, deemph, a, rate_out, rate_out2, nco, mode, output_scale, level, conseq, zero)


def want_for(iq, block_len, prm, hits=None, backend="oracle"):
    return chan_modes_stream(iq, block_len, prm.bin_e, prm.first_bin, prm.n_channels, prm.custom_atan, prm.mode, prm.output_scale or 1,
                             prm.squelch_level, prm.conseq_squelch, prm.squelch_zero, prm.deemph, prm.deemph_a, prm.rate_out, prm.rate_out2,
                             prm.nco, hits=hits, backend=backend)


GEOMETRIES = [
    (10, 384, 256, 2 * 131072, 2),        # the bench shape
    (10, 900, 256, 2 * 8192, 4),          # channel range wrapping through bin 0
    (5, 3, 20, 2 * 1024, 3),              # bin_e = 5
    (12, 100, 7, 2 * 8192, 4),            # two windows per block
]


@pytest.mark.parametrize("bin_e,first_bin,n_channels,block_len,n_blocks", GEOMETRIES)
@pytest.mark.parametrize("mode,scale", [(1, 1), (1, 3), (2, 1), (2, 3), (3, 1), (3, 3), (4, 0)])
def test_modes_bit_exact(bin_e, first_bin, n_channels, block_len, n_blocks, mode, scale):
    """am / usb / lsb (output_scale 1, and 3: int16 wraps) / raw on an FM signal and full-scale noise, two runs (carries cross a run boundary)"""
    prm = params(bin_e, first_bin, n_channels, mode=mode, output_scale=scale)
    for iq in (sig_fm(n_blocks * block_len // 2, seed=80, amp=9000), sig_noise(n_blocks * block_len, seed=81)):
        want = want_for(iq, block_len, prm)
        check(gpu_modes(iq, block_len, prm, n_runs=2), want, "mode %d" % mode)
        if have_ref() and n_channels <= 64:
            ref = want_for(iq, block_len, prm, backend="ref")
            assert all(np.array_equal(ref[k], want[k]) for k in want)


BURST = (10, 0, 128, 2 * 16384, 24)       # 16 windows per block, 24 blocks


@pytest.mark.parametrize("mode,custom_atan", [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("conseq", [0, 2, 10])
@pytest.mark.parametrize("zero", [0, 1])
@pytest.mark.parametrize("set_hits", [False, True])
def test_squelch_and_gate_on_bursts(mode, custom_atan, conseq, zero, set_hits):
    """carriers keyed per block: verdicts mixed per channel; FM -A std / -A fast and AM, -t 0 / 2 / 10, dropped or zeroed, the default count
    (11) and a set one"""
    bin_e, first_bin, n_ch, block_len, n_blocks = BURST
    iq, level = burst_capture(n_blocks, block_len, bin_e, first_bin, n_ch, seed=31)
    hits = np.random.RandomState(3).randint(0, 13, size=n_ch).astype(np.int32) if set_hits else None
    prm = params(bin_e, first_bin, n_ch, custom_atan, mode=mode, level=level, conseq=conseq, zero=zero)
    want = want_for(iq, block_len, prm, hits=hits)
    assert want["gate"].any() and (want["gate"] == 0).any()
    check(gpu_modes(iq, block_len, prm, n_runs=3, hits=hits), want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bin_e,n_ch,block_len,n_blocks,rate_out2", [(10, 64, 2 * 16384, 24, 8000), (10, 64, 2 * 16384, 24, -1),
                                                                     (4, 8, 2 * 65536, 6, 8000)])
def test_squelch_zero_behind_the_audio_stages(mode, bin_e, n_ch, block_len, n_blocks, rate_out2):
    """de-emphasis (and low_pass_real) on, squelch_zero: the zeroed ranges are the gated blocks' resampled outputs; the long rows take the
    segmented audio kernels"""
    iq, level = burst_capture(n_blocks, block_len, bin_e, 0, n_ch, seed=32)
    prm = params(bin_e, 0, n_ch, 1, 1, 7, 19531, rate_out2, mode=mode, level=level, conseq=0, zero=1)
    want = want_for(iq, block_len, prm)
    assert (want["gate"] == 2).any()
    check(gpu_modes(iq, block_len, prm, n_runs=2), want)


def test_nco_mode_am_with_squelch():
    bin_e, first_bin, n_ch, block_len, n_blocks = 8, 200, 64, 2 * 4096, 12
    iq, level = burst_capture(n_blocks, block_len, bin_e, first_bin, n_ch, seed=33, nco=1)
    prm = params(bin_e, first_bin, n_ch, 1, nco=1, mode=R.RXGPU_MODE_AM, output_scale=3, level=level, conseq=1, zero=1)
    want = want_for(iq, block_len, prm)
    assert want["gate"].any()
    check(gpu_modes(iq, block_len, prm, n_runs=2), want)


@pytest.mark.parametrize("mode,custom_atan", [(0, 1), (0, 0), (1, 1)])
def test_runs_chain_squelch_hits_and_reports(mode, custom_atan):
    """three synchronous runs == one run == three runs in flight (two at a time, squelch_hits chained on the device), reports in block order"""
    bin_e, first_bin, n_ch, block_len, n_blocks = BURST
    iq, level = burst_capture(n_blocks, block_len, bin_e, first_bin, n_ch, seed=34)
    prm = params(bin_e, first_bin, n_ch, custom_atan, mode=mode, level=level, conseq=2, zero=0)
    want = want_for(iq, block_len, prm)
    check(gpu_modes(iq, block_len, prm, n_runs=1), want, "one run")
    check(gpu_modes(iq, block_len, prm, n_runs=3), want, "three runs")
    check(gpu_modes(iq, block_len, prm, n_runs=3, how="async"), want, "three runs in flight")


@pytest.mark.parametrize("flag_all", ["1", "2"])
@pytest.mark.parametrize("custom_atan", [0, 1])
def test_squelch_with_host_fixups_forced(monkeypatch, flag_all, custom_atan):
    """$RXGPU_FLAG_ALL hands every libm sample to the host: its re-evaluation reads the squelched (zeroed) bins"""
    monkeypatch.setenv("RXGPU_FLAG_ALL", flag_all)
    bin_e, first_bin, n_ch, block_len, n_blocks = 10, 0, 24, 2 * 16384, 12
    iq, level = burst_capture(n_blocks, block_len, bin_e, first_bin, n_ch, seed=35)
    prm = params(bin_e, first_bin, n_ch, custom_atan, level=level, conseq=1, zero=1)
    want = want_for(iq, block_len, prm)
    got = gpu_modes(iq, block_len, prm, n_runs=2)
    assert got[6] > 0
    check(got, want)
    R.lib().rxgpu_knobs_reload()


def test_all_new_fields_zero_is_todays_fused_fm():
    """mode FM, squelch off at a fused geometry: today's output, carries untouched by the gate (11), an empty report"""
    bin_e, first_bin, n_ch, block_len, n_blocks = 9, 17, 100, 2 * 16384, 5
    iq = sig_fm(n_blocks * block_len // 2, seed=70, amp=9000)
    want, want_pre, _ = oracle_chan_stream(iq, block_len, bin_e, first_bin, n_ch, 1)
    rows, pre, _, hits, sr, gate, _, _ = gpu_modes(iq, block_len, params(bin_e, first_bin, n_ch, 1), n_runs=1)
    assert np.array_equal(rows, want) and np.array_equal(pre, want_pre)
    assert np.all(hits == 11) and not sr.any() and not gate.any()
    if have_ref():
        ref_out, ref_pre, _ = ref_chan_stream(iq, block_len, bin_e, first_bin, n_ch, 1)
        assert np.array_equal(rows, ref_out) and np.array_equal(pre, ref_pre)



@pytest.mark.parametrize("bin_e,first_bin,n_ch,block_len,n_blocks,n_runs,how,what", [
    (10, 0, 64, 2 * 16384, 64, 2, "sync", "32 blocks per run: k_ch_gate's sixteen-verdict walk"),
    (10, 0, 64, 2 * 16384, 48, 3, "async", "16 blocks per run, in flight: the same walk chained on the device"),
    (12, 100, 7, 2 * 8192, 12, 2, "sync", "two windows per block: k_ch_squelch<false>"),
    (11, 2000, 5, 2 * 2048, 10, 2, "sync", "one window per block"),
    (4, 0, 8, 2 * 16384, 8, 2, "sync", "1024 windows per block: k_ch_squelch_wave"),
])
@pytest.mark.parametrize("mode,zero", [(0, 0), (1, 1)])
def test_squelch_kernel_forms(bin_e, first_bin, n_ch, block_len, n_blocks, n_runs, how, what, mode, zero):
    """every form of the squelch and gate kernels the geometry picks, on bursts"""
    iq, level = burst_capture(n_blocks, block_len, bin_e, first_bin, n_ch, seed=36)
    prm = params(bin_e, first_bin, n_ch, 1, mode=mode, level=level, conseq=1, zero=zero)
    want = want_for(iq, block_len, prm)
    assert want["gate"].any() and (want["gate"] == 0).any(), what
    check(gpu_modes(iq, block_len, prm, n_runs=n_runs, how=how), want, what)


def test_pipelined_runs_without_wait_keep_host_memory_bounded():
    """a caller streaming with run_async and never waiting: host memory does not grow with the runs (the verdicts of a run that run_async
    retires on its own are not kept), and the next wait reports exactly the two runs it retired, as the synchronous runs did"""
    from gpu_support import to_dev, torch_cuda
    torch = torch_cuda()
    bin_e, n_ch, block_len, nb, runs = 8, 256, 2 * 256, 1024, 450        # 1024 blocks of one window per run: 1.3 MB of sr / gate per run
    rs = np.random.RandomState(37)
    iq = (rs.randint(-3000, 3000, size=nb * block_len) * np.repeat(rs.randint(0, 2, size=nb), block_len)).astype(np.int16)
    d_iq = to_dev(iq)
    d_out = torch.zeros((n_ch, nb), dtype=torch.int16, device="cuda")
    prm = params(bin_e, 0, n_ch, 1, level=5, conseq=1, zero=0)
    rss = lambda: int(open("/proc/self/statm").read().split()[1]) * 4096
    reports = {}
    for how in ("async", "sync"):
        ch = R.Channeliser(prm, nb, block_len, R.sine_table(bin_e))
        last = []
        for i in range(runs):
            if how == "async":
                ch.run_async(d_iq.data_ptr(), nb, block_len, d_out.data_ptr(), nb)
                if i == 150:                  # the HIP runtime grows its own pools once in the first hundred runs in flight: measured after them
                    r0 = rss()
            else:
                ch.run(d_iq.data_ptr(), nb, block_len, d_out.data_ptr(), nb)
                last = (last + [ch.squelch_report(nb)])[-2:]
        if how == "async":
            grew = rss() - r0
            assert grew < 16 << 20, "host memory grew by %d bytes over %d runs in flight" % (grew, runs - 150)
            ch.wait()
            with pytest.raises(R.RxGpuError):
                ch.squelch_report(runs * nb)
            reports[how] = ch.squelch_report(2 * nb)
        else:
            reports[how] = tuple(np.concatenate([r[k] for r in last], axis=1) for k in range(2))
        reports[how + "_hits"] = ch.get_squelch_carry()
        ch.close()
    assert reports["async"][1].any() and (reports["async"][1] == 0).any()
    for k in range(2):
        assert np.array_equal(reports["async"][k], reports["sync"][k])
    assert np.array_equal(reports["async_hits"], reports["sync_hits"])
