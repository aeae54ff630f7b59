#!/usr/bin/env python3
"""Times the evaluation loop's device pieces at BASELINE config-3 scale (256 utterances x 512 frames = 65,664 samples):
rced_mix_snr and rced_sdr through the C ABI with HIP events on the launch stream (>= 20 warm-ups, >= 100 runs, the median
of per-run times), beside the HBM floor their byte counts imply; and FullyCNNTester.evaluate_pcm's device part against
the same chain without the score (stft_batch -> model -> istft_batch): the difference is what scoring costs.
STOI (rced_stoi) is timed at the same shape, beside the wall time of its float64 numpy / scipy restatement
(tests/stoi_np.py) for the same batch on 16 host processes.  `python tools/time_eval.py stoi` times STOI alone.
The further scores -- legs `estoi`, `stoi+estoi` (one rced_stoi_ex call for both), `si_sdr`, `seg_snr` -- run at the same shape
beside their restatements (tests/estoi_np.py, tests/td_metrics_np.py) on the same 16 processes, with the ratio of `stoi+estoi`
to rced_stoi alone in this process; `python tools/time_eval.py ext` times those alone.
LLR and WSS (rced_llr, rced_wss) -- legs `llr`, `wss` -- run at the same shape beside their restatement (tests/sepm_np.py) on the
same 16 processes, and so do fwSNRseg and CD (rced_fwseg, rced_cepd; legs `fw_seg_snr`, `cd`; tests/sepm2_np.py);
`python tools/time_eval.py sepm` times those four alone.
The SDR of BSS Eval (rced_bss_sdr, 512 taps) -- leg `bss_sdr` -- runs at the same shape beside its restatement (tests/bsseval_np.py,
the normal equations) on the same 16 processes; `python tools/time_eval.py bss` times it alone, with WSS and STOI from the same run.
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from fullycnnspeechenhancement_amd import audio, build_model  # noqa: E402
from fullycnnspeechenhancement_amd import weights as _weights  # noqa: E402

N, T = 256, 512
L = (T - 1) * 128 + 256
COPY_TBPS = 6.29          # measured device copy rate (read + write bytes)
WARMUP, RUNS = 20, 100


def timed_us(fn):
    """Median device time of fn() in microseconds: one event pair per run, the L2 / Infinity Cache left as the previous run left it."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RUNS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "p90_us": ts[int(0.9 * len(ts))]}


HOST_PROCS = 16


# leg -> (module under tests/, function, arguments after the pair): the float64 restatement a device leg is set beside
RESTATEMENTS = {"stoi": ("stoi_np", "stoi", (8000,)), "estoi": ("estoi_np", "estoi", (8000,)), "si_sdr": ("td_metrics_np", "si_sdr", ()),
                "seg_snr": ("td_metrics_np", "seg_snr", (8000,)), "llr": ("sepm_np", "llr", (8000,)), "wss": ("sepm_np", "wss", (8000,)),
                "bss_sdr": ("bsseval_np", "bss_sdr", (512,)), "fw_seg_snr": ("sepm2_np", "fwseg", (8000,)), "cd": ("sepm2_np", "cd", (8000,))}
# command-line leg -> the restatements it runs; no leg: all of them
HOST_LEGS = {"stoi": ("stoi",), "bss": ("bss_sdr",), "ext": ("estoi", "si_sdr", "seg_snr"), "sepm": ("llr", "wss", "fw_seg_snr", "cd")}


def _host_score(job):
    leg, seed = job
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import importlib
    import numpy as np
    module, fn, rest = RESTATEMENTS[leg]
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal(L)
    return getattr(importlib.import_module(module), fn)(x, x + 0.05 * rng.standard_normal(L), *rest)


def host_seconds(leg):
    """Wall time of a leg's restatement over N utterances of L samples on HOST_PROCS processes (forked before the GPU is touched)."""
    import multiprocessing
    import time
    with multiprocessing.get_context("fork").Pool(HOST_PROCS) as pool:
        pool.map(_host_score, [(leg, seed) for seed in range(HOST_PROCS)])      # imports and first-call costs
        t0 = time.perf_counter()
        pool.map(_host_score, [(leg, seed) for seed in range(N)], chunksize=1)
        return time.perf_counter() - t0


def beside(out, host, legs):
    """`out` with each leg's restatement wall time next to its device time."""
    for leg in legs:
        out[leg + "_host_restatement_s"] = {"seconds": host[leg], "processes": HOST_PROCS}
    return out


def stoi_timings(speech, mix, host):
    out = {"stoi": timed_us(lambda: audio.stoi_batch(speech, mix)),
           "stoi_single_utterance": timed_us(lambda: audio.stoi_batch(speech[:1], mix[:1]))}
    return beside(out, host, HOST_LEGS["stoi"])


def ext_timings(speech, mix, host):
    """The four further legs, each beside its restatement's wall time, and stoi+estoi over rced_stoi alone (same process)."""
    out = {"estoi": timed_us(lambda: audio.stoi_batch(speech, mix, extended=True)),
           "stoi+estoi": timed_us(lambda: audio.stoi_batch(speech, mix, extended="both")),
           "si_sdr": timed_us(lambda: audio.si_sdr_batch(speech, mix)),
           "seg_snr": timed_us(lambda: audio.seg_snr_batch(speech, mix))}
    alone = timed_us(lambda: audio.stoi_batch(speech, mix))
    out["stoi_alone_same_process"] = alone
    out["stoi+estoi_over_stoi"] = out["stoi+estoi"]["median_us"] / alone["median_us"]
    return beside(out, host, HOST_LEGS["ext"])


def sepm_timings(speech, mix, host):
    """LLR, WSS, fwSNRseg and CD, each beside its restatement's wall time."""
    out = {"llr": timed_us(lambda: audio.llr_batch(speech, mix)), "wss": timed_us(lambda: audio.wss_batch(speech, mix)),
           "fw_seg_snr": timed_us(lambda: audio.fw_seg_snr_batch(speech, mix)), "cd": timed_us(lambda: audio.cep_dist_batch(speech, mix))}
    return beside(out, host, HOST_LEGS["sepm"])


def bss_timings(speech, mix, host):
    """BSS Eval's SDR at 512 taps (and at one tap: what the 512 lags cost) beside its restatement's wall time."""
    out = {"bss_sdr": timed_us(lambda: audio.bss_sdr_batch(speech, mix)),
           "bss_sdr_one_tap": timed_us(lambda: audio.bss_sdr_batch(speech, mix, filter_length=1)),
           "bss_sdr_single_utterance": timed_us(lambda: audio.bss_sdr_batch(speech[:1], mix[:1]))}
    return beside(out, host, HOST_LEGS["bss"])


TIMINGS = {"stoi": stoi_timings, "ext": ext_timings, "sepm": sepm_timings, "bss": bss_timings}


def main():
    leg = sys.argv[1] if len(sys.argv) == 2 and sys.argv[1] in TIMINGS else None
    host = {name: host_seconds(name) for group in ([leg] if leg else HOST_LEGS) for name in HOST_LEGS[group]}     # first: these fork
    g = torch.Generator(device="cuda").manual_seed(1)
    speech = torch.randn((N, L), device="cuda", generator=g) * 0.1
    noise = torch.randn((N, L), device="cuda", generator=g) * 0.05
    out = {"N": N, "L": L}
    if leg:
        mix = audio.mix_snr_batch(speech, noise, 5.0)
        out.update(TIMINGS[leg](speech, mix, host))
        if leg == "bss":
            out["wss"], out["stoi"] = timed_us(lambda: audio.wss_batch(speech, mix)), timed_us(lambda: audio.stoi_batch(speech, mix))
        print(json.dumps(out))
        return

    # the mix reads speech and noise twice and writes once; the SDR reads two signals once
    mix_bytes, sdr_bytes = 5 * N * L * 4, 2 * N * L * 4
    r = timed_us(lambda: audio.mix_snr_batch(speech, noise, 5.0))
    r.update(bytes=mix_bytes, floor_us=mix_bytes / COPY_TBPS / 1e6)
    r["fraction_of_floor"] = r["floor_us"] / r["median_us"]
    out["mix_snr_equal_lengths"] = r

    short = noise[:, :24000].contiguous()                      # tiled: ls / ln = 2.7, two gains
    gains = torch.rand((N, 2), dtype=torch.float64, device="cuda") * 2
    r = timed_us(lambda: audio.mix_snr_batch(speech, short, 5.0, gains=gains))
    r.update(bytes=(3 * N * L + 2 * N * 24000) * 4)
    out["mix_snr_tiled_noise"] = r

    mix = audio.mix_snr_batch(speech, noise, 5.0)
    r = timed_us(lambda: audio.sdr_batch(speech, mix))
    r.update(bytes=sdr_bytes, floor_us=sdr_bytes / COPY_TBPS / 1e6)
    r["fraction_of_floor"] = r["floor_us"] / r["median_us"]
    out["sdr"] = r

    one = speech[:1].contiguous()                              # N = 1: a long signal alone (33 workgroups)
    out["sdr_single_utterance"] = timed_us(lambda: audio.sdr_batch(one, mix[:1]))

    for group in ("stoi", "ext", "sepm", "bss"):
        out.update(TIMINGS[group](speech, mix, host))

    model = build_model("FullyCNNV3", False, weights=_weights.synthetic_weights(3, seed=42))
    lens = [L] * N

    def chain():
        mag, ph = audio.stft_batch(mix, lens)
        return audio.istft_batch(model(mag), ph)

    out["chain_stft_model_istft"] = timed_us(chain)
    out["chain_with_sdr"] = timed_us(lambda: audio.denoise_and_score(model, mix, speech, lens))
    out["scoring_cost_us"] = out["chain_with_sdr"]["median_us"] - out["chain_stft_model_istft"]["median_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
