"""The channeliser's demodulators, power squelch and demod-thread gate (rxgpu_chan_params.mode .. squelch_zero) as the reference chain,
driven from Python callback block after callback block: every channel's block of bins through full_demod (rtl_fm.c:759-824) with one
demod_state configuration and the channel's own carries, then the demod thread's gate (rtl_fm.c:927-940).

Two backends, one interface:
  "ref"     reference-BUILT code only (oracle/_ref): its fix_fft per window (ref_power_chan_windows), its global demod_state, its own
            full_demod, rms, low_pass and deemph_filter (the de-emphasis static forced and read back as oracle/ref_fm_shim.c does)
  "oracle"  the CPU restatement (oracle/rx_oracle.c: rxo_fix_fft, rxo_fm_full_demod, rxo_rms, rxo_low_pass), held to "ref" by
            tests/test_chan_modes_host.py; it needs nothing outside the repository, so the GPU tests use it everywhere
"""
import ctypes as C

import numpy as np

from support import oracle, ref_fm, ref_power, ptr16, i16p, intp, FmState

# librxgpu / oracle mode numbers (0 fm, 1 am, 2 usb, 3 lsb, 4 raw) -> ref_fm_fn's (0 fm, 1 raw, 2 am, 3 usb, 4 lsb)
REF_FN = {0: 0, 1: 2, 2: 3, 3: 4, 4: 1}


def demod_thread_gate(hits, level, conseq, zero):
    """rtl_fm.c:928-940 (a static thread function, restated): squelch_hits after the gate, and 0 written / 1 dropped / 2 zeroed"""
    active = bool(level) and hits > conseq
    if active and not zero:
        return conseq + 1, 1                     # hair trigger
    return hits, (2 if active else 0)


def _fix_mpy(a, b):
    return ((((a * b) >> 14) + 1) >> 1).astype(np.int16).astype(np.int32)


class _Backend:
    def __init__(self, name, bin_e):
        self.name, self.bin_e, self.n = name, bin_e, 1 << bin_e
        if name == "ref":
            from rx_tools_amd.structs import DemodState
            self.P, self.F = ref_power(), ref_fm()
            self.P.ref_power_chan_windows.argtypes = [i16p, C.c_int, C.c_int, C.c_int, C.c_int, i16p]
            self.F.rms.argtypes = [i16p, C.c_int, C.c_int]
            self.F.ref_fm_scale_block.argtypes = [i16p, C.c_uint32, i16p]
            self.F.ref_fm_scale_block.restype = None
            self.P.sine_table.argtypes = [C.c_int]
            self.d = DemodState.from_address(self.F.ref_fm_demod())
            self.tmp = DemodState()              # low_pass in front of rms (NCO mode) and the de-emphasis peek
        else:
            self.O = oracle()
            self.O.rxo_fix_fft.argtypes = [i16p, C.c_int, i16p]
            self.O.rxo_sine_table.argtypes = [C.c_int, i16p]
            self.O.rxo_rms.argtypes = [i16p, C.c_int, C.c_int]
            self.O.rxo_low_pass.argtypes = [i16p, C.c_int, C.c_int, intp, intp, intp]

    def sinewave(self):
        n = self.n
        if self.name == "ref":
            self.P.sine_table(self.bin_e)
            return np.ctypeslib.as_array(self.P.ref_power_sinewave(), shape=(3 * n // 4,)).astype(np.int32)
        sw = np.zeros(3 * n // 4, np.int16)
        self.O.rxo_sine_table(self.bin_e, ptr16(sw))
        return sw.astype(np.int32)

    def bins(self, blk, wpb, first_bin, n_channels):
        """[n_channels][2 wpb] int16: bin first_bin + c of every window of the block (fix_fft, rtl_power.c:264-320)"""
        lp = np.zeros((n_channels, 2 * wpb), np.int16)
        if self.name == "ref":
            assert self.P.ref_power_chan_windows(ptr16(blk), wpb, self.bin_e, first_bin, n_channels, ptr16(lp)) == 0
            return lp
        sw = self.sinewave().astype(np.int16)
        win = blk.reshape(wpb, 2 * self.n).copy()
        for w in range(wpb):
            row = win[w]
            self.O.rxo_fix_fft(ptr16(row), self.bin_e, ptr16(sw))
        b = (first_bin + np.arange(n_channels)) & (self.n - 1)
        lp[:, 0::2] = win[:, 2 * b].T
        lp[:, 1::2] = win[:, 2 * b + 1].T
        return lp

    def mixed(self, blk, wpb, first_bin, n_channels):
        """NCO mode: [n_channels][len(blk)] the callback-scaled block (rtl_fm.c:845-848) mixed by each channel's NCO, products by FIX_MPY"""
        n, h = self.n, self.n // 2
        if self.name == "ref":
            scaled = np.zeros(len(blk), np.int16)
            self.F.ref_fm_scale_block(ptr16(blk), len(blk), ptr16(scaled))
        else:
            scaled = np.trunc(blk.astype(np.float64) / 32767.0 * 128.0 + 0.4).astype(np.int16)    # rxo_scale_sample
        sw = self.sinewave()
        xr = scaled[0::2].astype(np.int32).reshape(wpb, n)
        xi = scaled[1::2].astype(np.int32).reshape(wpb, n)
        out = np.zeros((n_channels, len(blk)), np.int16)
        idx = np.arange(n)
        for c in range(n_channels):
            k = (first_bin + c) & (n - 1)
            p = (k * idx) & (n - 1)
            q = p & (h - 1)
            co = np.where(p >= h, -sw[q + n // 4], sw[q + n // 4])
            si = np.where(p >= h, -sw[q], sw[q])
            out[c, 0::2] = (_fix_mpy(xr, co) + _fix_mpy(xi, si)).astype(np.int16).reshape(-1)
            out[c, 1::2] = (_fix_mpy(xi, co) - _fix_mpy(xr, si)).astype(np.int16).reshape(-1)
        return out

    def rms_of_decimated(self, lp, ds):
        """full_demod's sr (rtl_fm.c:781): rms over the block after low_pass at downsample ds"""
        if self.name == "ref":
            t = self.tmp
            C.memmove(C.addressof(t.lowpassed), lp.ctypes.data, lp.nbytes)
            t.lp_len = len(lp)
            if ds > 1:
                t.downsample = ds
                t.now_r = t.now_j = t.prev_index = 0
                self.F.low_pass(C.byref(t))
            return self.F.rms(C.cast(C.addressof(t.lowpassed), i16p), t.lp_len, 1)
        x = lp.copy()
        m = len(x)
        if ds > 1:
            a, b, i = C.c_int(0), C.c_int(0), C.c_int(0)
            m = self.O.rxo_low_pass(ptr16(x), m, ds, C.byref(a), C.byref(b), C.byref(i))
        return self.O.rxo_rms(ptr16(x), m, 1)

    def full_demod(self, lp, ds, cfg, pre, audio, hits):
        """one channel's block through full_demod: returns (result, (pre_r, pre_j), [avg, now_lpr, prev_lpr_index], squelch_hits)"""
        if self.name == "ref":
            F, d = self.F, self.d
            d.downsample, d.downsample_passes, d.post_downsample = ds, 0, 1
            d.mode_demod = F.ref_fm_fn(REF_FN[cfg["mode"]])
            d.output_scale = cfg["output_scale"]
            d.squelch_level, d.squelch_hits = cfg["squelch_level"], int(hits)
            d.custom_atan, d.deemph, d.deemph_a = cfg["custom_atan"], cfg["deemph"], cfg["a"]
            d.rate_in = d.rate_out = cfg["rate_out"]
            d.rate_out2, d.dc_block_audio = cfg["rate_out2"], 0
            d.now_r = d.now_j = d.prev_index = 0
            d.pre_r, d.pre_j = int(pre[0]), int(pre[1])
            d.now_lpr, d.prev_lpr_index = int(audio[1]), int(audio[2])
            C.memmove(C.addressof(d.lowpassed), lp.ctypes.data, lp.nbytes)
            d.lp_len = len(lp)
            if cfg["deemph"]:
                assert F.ref_fm_deemph_force(int(audio[0])) == audio[0]
            F.full_demod(C.byref(d))
            avg = audio[0]
            if cfg["deemph"]:                    # ref_fm_shim.c's peek: a = 2^20 on one zero sample leaves avg unchanged in result[0]
                t = self.tmp
                t.deemph_a, t.result_len, t.result[0] = 1 << 20, 1, 0
                F.deemph_filter(C.byref(t))
                avg = t.result[0]
            res = np.ctypeslib.as_array(d.result)[:d.result_len].copy()
            return res, (d.pre_r, d.pre_j), [avg, d.now_lpr, d.prev_lpr_index], d.squelch_hits
        st = FmState()
        st.downsample, st.downsample_passes, st.post_downsample = ds, 0, 1
        st.mode, st.output_scale = cfg["mode"], cfg["output_scale"]
        st.squelch_level, st.squelch_hits = cfg["squelch_level"], int(hits)
        st.custom_atan, st.deemph, st.deemph_a = cfg["custom_atan"], cfg["deemph"], cfg["a"]
        st.rate_out, st.rate_out2 = cfg["rate_out"], cfg["rate_out2"]
        st.pre_r, st.pre_j = int(pre[0]), int(pre[1])
        st.deemph_avg, st.now_lpr, st.prev_lpr_index = int(audio[0]), int(audio[1]), int(audio[2])
        x = lp.copy()
        n = C.c_int(len(x))
        out = np.zeros(len(x) + 16, np.int16)
        k = self.O.rxo_fm_full_demod(C.byref(st), ptr16(x), C.byref(n), ptr16(out))
        return out[:k].copy(), (st.pre_r, st.pre_j), [st.deemph_avg, st.now_lpr, st.prev_lpr_index], st.squelch_hits


def burst_capture(n_blocks, block_len, bin_e, first_bin, n_channels, seed, nco=0):
    """carriers keyed on and off per block (a random pattern per carrier) over weak noise, and a squelch level that splits the
    (channel, block) verdicts about evenly: (iq, level)"""
    from support import sig_noise
    rs = np.random.RandomState(seed)
    n = 1 << bin_e
    T = n_blocks * block_len // 2
    t = np.arange(T)
    x = sig_noise(2 * T, seed=seed, amp=60).astype(np.float64)
    for k in first_bin + rs.choice(n_channels, size=min(12, n_channels), replace=False):
        on = np.repeat(rs.randint(0, 2, size=n_blocks), block_len // 2)
        ph = 2 * np.pi * (k + 0.3) / n * t + rs.uniform(0, 6.28)
        amp = rs.uniform(1500, 4000)
        x[0::2] += on * amp * np.cos(ph)
        x[1::2] += on * amp * np.sin(ph)
    iq = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    sr = chan_modes_stream(iq, block_len, bin_e, first_bin, n_channels, squelch_level=1, nco=nco)["sr"]
    return iq, int(np.median(sr)) + 1


def chan_modes_stream(iq, block_len, bin_e, first_bin, n_channels, custom_atan=1, mode=0, output_scale=1, squelch_level=0, conseq_squelch=0,
                      squelch_zero=0, deemph=0, a=0, rate_out=0, rate_out2=-1, nco=0, pre=None, audio=None, hits=None, backend="oracle"):
    """The channeliser's stream through the reference chain.  Returns a dict: out [n_channels][samples] (every block's result, zeros where the
    gate zeroed it; raw: the int16 I, Q pairs), pre [2 n_channels], audio [n_channels][3], hits [n_channels], sr and gate [n_channels][n_blocks]
    (sr as full_demod computed it, 0 with the squelch off; gate 0 written / 1 dropped / 2 zeroed)."""
    B = _Backend(backend, bin_e)
    n = 1 << bin_e
    n_blocks = len(iq) // block_len
    wpb = block_len // 2 // n
    ds = n if nco else 1
    cfg = dict(mode=mode, output_scale=output_scale, squelch_level=squelch_level, custom_atan=custom_atan, deemph=deemph, a=a,
               rate_out=rate_out, rate_out2=rate_out2)
    pre = np.zeros(2 * n_channels, np.int32) if pre is None else np.array(pre, np.int32).copy()
    audio = np.zeros((n_channels, 3), np.int32) if audio is None else np.array(audio, np.int32).reshape(n_channels, 3).copy()
    hits = np.full(n_channels, 11, np.int32) if hits is None else np.array(hits, np.int32).copy()      # demod_init, rtl_fm.c:1091
    sr = np.zeros((n_channels, n_blocks), np.int32)
    gate = np.zeros((n_channels, n_blocks), np.uint8)
    outs = [[] for _ in range(n_channels)]
    for b in range(n_blocks):
        blk = np.ascontiguousarray(iq[b * block_len:(b + 1) * block_len])
        lps = B.mixed(blk, wpb, first_bin, n_channels) if nco else B.bins(blk, wpb, first_bin, n_channels)
        for c in range(n_channels):
            lp = np.ascontiguousarray(lps[c])
            if squelch_level:
                sr[c, b] = B.rms_of_decimated(lp, ds)
            res, p, au, h = B.full_demod(lp, ds, cfg, pre[2 * c:2 * c + 2], audio[c], hits[c])
            pre[2 * c], pre[2 * c + 1] = p
            audio[c] = au
            hits[c], gate[c, b] = demod_thread_gate(h, squelch_level, conseq_squelch, squelch_zero)
            if gate[c, b] == 2:
                res[:] = 0
            outs[c].append(res)
    out = np.stack([np.concatenate(o) if o else np.zeros(0, np.int16) for o in outs])
    return dict(out=out, pre=pre, audio=audio, hits=hits, sr=sr, gate=gate)
