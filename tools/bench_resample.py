#!/usr/bin/env python3
"""Times the sample-rate conversion (rced_resample) at BASELINE config-5 scale: 256 rows -> 65,664 samples at
8 kHz each (512 frames), from 16 kHz mono (int16 and float32), 48 kHz stereo int16 and 44.1 kHz mono int16, into padded float32 rows and --
corpus ingest -- packed into one arena through audio.resample_arena's packed mode (its launch timed alone: the C entry on
device-resident plans).

HIP events around every single call, 20 warm-ups, the median of 100.  Beside each time: the fp64 FMAs it implies (outputs x
taps per phase), the bytes read and written and what they cost at the 6.29 TB/s copy rate DESIGN.md uses.  --host adds the
float64 restatement (tests/resample_np.py: the direct sum in numpy) and scipy.signal.resample_poly with the same filter over
the same 256 rows from 16 kHz, on 16 processes.  One JSON line per case."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

N, LOUT, WARM, REPS, COPY_TBS = 256, 65664, 20, 100, 6.29


def host_row(args):
    import resample_np as R
    seed, form = args
    x = np.random.RandomState(seed).uniform(-1, 1, 2 * LOUT)
    return (R.resample if form == "sum" else R.scipy_form)(x, 16000, 8000).size


def host_times():
    from multiprocessing import Pool
    out = {}
    with Pool(16) as pool:
        pool.map(host_row, [(i, "poly") for i in range(16)])           # imports done
        for form, rows in (("sum", 32), ("poly", N)):                    # the direct sum: 32 rows, scaled to 256
            t0 = time.perf_counter()
            pool.map(host_row, [(i, form) for i in range(rows)])
            out["host16_%s_s" % form] = (time.perf_counter() - t0) * N / rows
    return out


def main():
    host = host_times() if "--host" in sys.argv else None       # before this process opens the GPU: the workers never see it
    import torch
    from fullycnnspeechenhancement_amd import _lib, audio
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    for name, rate, channels, dtype in (("16k_s16", 16000, 1, np.int16), ("16k_f32", 16000, 1, np.float32),
                                        ("48k_s16x2", 48000, 2, np.int16), ("44k1_s16", 44100, 1, np.int16)):
        frames = -(-LOUT * rate // 8000)
        assert audio.resample_length(frames, rate, 8000) == LOUT
        if dtype == np.int16:
            src = torch.as_tensor(rng.integers(-20000, 20000, (N * frames, channels)).astype(np.int16), device="cuda")
        else:
            src = torch.as_tensor(rng.uniform(-1, 1, (N * frames, channels)).astype(np.float32), device="cuda")
        p, q, left, table = audio.resample_taps(rate, 8000)
        begins = torch.arange(N, dtype=torch.int64, device="cuda") * frames
        counts = torch.full((N,), frames, dtype=torch.int32, device="cuda")
        rows = torch.empty((N, LOUT), dtype=torch.float32, device="cuda")
        arena = torch.empty((N * LOUT,), dtype=torch.float32, device="cuda")
        obeg = torch.arange(N, dtype=torch.int64, device="cuda") * LOUT
        sd = _lib.PCM_S16 if dtype == np.int16 else _lib.PCM_F32

        def call(out, out_begins):
            _lib.check(lib.rced_resample(src.data_ptr(), sd, channels, N * frames, begins.data_ptr(), counts.data_ptr(), N, rate,
                                         8000, out.data_ptr(), _lib.PCM_F32, out_begins.data_ptr() if out_begins is not None else None,
                                         LOUT, LOUT, 0, st))

        res = {"case": name, "rows": N, "outputs_per_row": LOUT, "p": p, "q": q, "taps_per_phase": int(table.shape[1])}
        for mode, out, ob in (("rows", rows, None), ("packed", arena, obeg)):
            for _ in range(WARM):
                call(out, ob)
            torch.cuda.synchronize()
            ms = []
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(out, ob)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            res["%s_ms_median" % mode], res["%s_ms_min" % mode] = float(np.median(ms)), float(np.min(ms))
        assert torch.equal(rows.reshape(-1), arena)
        fma = N * LOUT * int(table.shape[1])
        nbytes = src.numel() * src.element_size() + rows.numel() * 4
        res.update(fp64_fma=fma, fp64_tfma_per_s=fma / (res["rows_ms_median"] * 1e-3) / 1e12, bytes=nbytes,
                   copy_floor_ms=nbytes / (COPY_TBS * 1e12) * 1e3)
        print(json.dumps(res), flush=True)
        del src, rows, arena
    if host is not None:
        print(json.dumps(host), flush=True)


if __name__ == "__main__":
    main()
