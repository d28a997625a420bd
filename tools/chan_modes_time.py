"""tools/chan_modes_time.py -- the channeliser's bench shape (bin_e 10, 256 channels from bin 384, 2048 callback blocks of 131 072 samples:
1 GiB per step) with the demodulators and the squelch: 20 pipelined steps after warm-up per configuration, one process, on a capture in which
about half of every channel's blocks are quiet; GSample/s and the ratio to FM -A fast (the fused path) of the same run.
`python tools/chan_modes_time.py [squelch]`: only the configuration named (under tools/prof_cmd.sh for its kernel table)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import rx_tools_amd as R
from bench import device_capture
L = R.lib(); R.check(L.rxgpu_init(0))
block_len, bin_e, n_ch, n_blocks, steps = 2 * 131072, 10, 256, 2048, 20
T = n_blocks * (block_len // 2)
d_iq = device_capture(torch, torch.device("cuda"), T, seed=4242, amp=600.0)
d_iq.view(n_blocks, block_len)[1::2] //= 64                   # every other callback block quiet
windows = T >> bin_e
d_out = torch.zeros((n_ch, 2 * windows), dtype=torch.int16, device="cuda")


def prm(custom_atan=1, mode=0, level=0, zero=0):
    return R.ChanParams(bin_e, 384, n_ch, custom_atan, 0, 0, 0, -1, 0, mode, 1, level, 0, zero)


# the squelch level: between the quiet and the loud blocks' rms (full_demod's sr as the library reports it)
ch = R.Channeliser(prm(level=1), n_blocks, block_len, R.sine_table(bin_e))
ch.run(d_iq.data_ptr(), n_blocks, block_len, d_out.data_ptr(), 2 * windows)
sr, _ = ch.squelch_report(n_blocks)
ch.close()
level = int(np.median(sr)) + 1
configs = [("fm -A fast", prm()), ("squelch: fm -A fast", prm(level=level)), ("squelch: fm -A std", prm(0, level=level)),
           ("am", prm(mode=R.RXGPU_MODE_AM)), ("squelch: am, squelch_zero", prm(mode=R.RXGPU_MODE_AM, level=level, zero=1)),
           ("raw", prm(mode=R.RXGPU_MODE_RAW))]
if len(sys.argv) > 1:
    configs = [c for c in configs if c[0].startswith(sys.argv[1])][:1]
print("squelch level", level, "quiet fraction", round(float((sr < level).mean()), 3), flush=True)
base = None
for label, p in configs:
    ch = R.Channeliser(p, n_blocks, block_len, R.sine_table(bin_e))
    for _ in range(10):
        ch.run(d_iq.data_ptr(), n_blocks, block_len, d_out.data_ptr(), 2 * windows)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.run_async(d_iq.data_ptr(), n_blocks, block_len, d_out.data_ptr(), 2 * windows)
    ch.wait()
    dt = (time.perf_counter() - t0) / steps
    gs = T / dt / 1e9
    base = base or gs
    _, gate = ch.squelch_report(2 * n_blocks) if p.squelch_level else (None, np.zeros(1))          # the two runs the wait retired
    print(label.ljust(28), "ms %.3f" % (dt * 1e3), "GS/s %.1f" % gs, "ratio %.3f" % (gs / base), "gated %.3f" % float((gate > 0).mean()), flush=True)
    ch.close()
