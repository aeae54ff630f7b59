#!/usr/bin/env python3
"""sha256 digests of what the audio kernel family computes (x6_dft.h and its users: kernels_audio_x6.h, kernels_stream.h,
kernels_stoi.h) and of what the resampling family computes (kernels_resample.h and its users: kernels_rstream.h, kernels_rfree.h;
streaming.py, freerun.py) on seeded inputs, one JSON line: run it once per library (RCED_LIB=exp/<name>.so, or the product) in
fresh processes -- and, for the Python half, once per checkout -- and compare the lines: a refactor of these kernels and of the
objects over them leaves every digest as it was.  Sections named as arguments run alone (default: all).  Seconds.
  stft / istft   kernels="x6" over the (N, T) table of tests/test_audio_edges_gpu.py (single block; split per 1; one workgroup
                 walking 2 or 3 blocks, T = 65 and 129: the fused ISTFT carries across a seam; split per 2 with an empty trailing
                 range), ragged lengths (1, 2, odd, 8319 / 8320 / 8321), STFT with and without phase, ISTFT of arbitrary spectra
                 (imaginary parts of bins 0 and 128 nonzero: slot 1 and the rank-1 term) at nfft 512 and 256
  stream         CR-CED with synthetic weights, 5 lanes, max_hops 8, nfft 512 and 256: pushes of 1, 3, 8, 3, 1 hops with a lane idle
                 on alternate pushes, lanes finishing at different pushes (tails of 0, 1, 127 samples; two with fewer than 5 hops
                 pushed: the head inside a finish) and reused afterwards
  stoi           the ragged 8-utterance batch of tests/test_stoi_gpu.py at 8 and 10 kHz, and an input under 30 spectral frames:
                 scores and the (F, K, M) detail
  resample       16000 -> 8000, 44100 -> 8000, 8000 -> 48000, 8000 -> 8000, each from int16 stereo to float32 and from float32 mono
                 to int16.  Offline: 4 ragged rows (0, 1, an odd number of frames, and the count that gives tile + 1 outputs, tile
                 from rced_rfree_plan), padded (resample_batch) and packed into an arena (resample_arena).  Unit lanes: 3
                 StreamingResampler lanes, pushes of 1 and max_units units with a lane idle on alternate pushes, started(),
                 finishes with tails of 0, 1 and unit_in - 1 frames, a reset, lanes reused.  Free lanes: 3 FreeResampler lanes
                 (one object with prefill > 0), pushes of 0, 1, 441 and max_frames frames, take None / partial / 0, a lane with a
                 negative count, a finish whose tail exceeds max_frames.  Chains: StreamingDenoiser(16000 -> 16000, int16) and
                 BlockDenoiser(block 441 at 44100), a few calls and a finish each, synthetic CR-CED weights"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))          # stoi_np: the signals of the STOI parity test
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fullycnnspeechenhancement_amd import audio, build_model  # noqa: E402
from fullycnnspeechenhancement_amd import weights as _weights  # noqa: E402

CASES = [(2, 1), (1, 2), (3, 63), (2, 64), (3, 65), (255, 65), (256, 65), (257, 128), (256, 129), (100, 257), (64, 321)]
OUT = {}


def digest(name, t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    OUT[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def dev(a):
    return torch.as_tensor(a, device="cuda")


def stft_istft():
    for N, T in CASES:
        L = 256 + 128 * (T - 1)
        rng = np.random.default_rng(1000 * N + T)
        special = [L, L - 77 if L > 77 else L, 1, 2, 131, 255, 257] + ([8319, 8320, 8321] if T > 64 else [])
        lens = [int(v) for v in rng.integers(1, L + 1, N)]
        for r, v in enumerate(special[:N]):
            lens[r] = min(v, L)
        pcm = (0.2 * rng.standard_normal((N, L))).astype(np.float32)
        pcm[np.arange(L)[None, :] >= np.asarray(lens)[:, None]] = 7.0      # junk past a length never gets in
        tag = "%dx%d" % (N, T)
        mag, ph = audio.stft_batch(dev(pcm), lens, frames=T)
        digest("stft/%s/mag" % tag, mag)
        digest("stft/%s/phase" % tag, torch.view_as_real(ph))
        digest("stft/%s/mag_only" % tag, audio.stft_batch(dev(pcm), lens, frames=T, with_phase=False)[0])
        smag = np.abs(rng.standard_normal((N, T, 129))).astype(np.float32)
        ang = rng.uniform(-np.pi, np.pi, (N, T, 129))
        sph = np.exp(1j * ang).astype(np.complex64)
        for nfft in (512, 256):
            digest("istft/%s/nfft%d" % (tag, nfft), audio.istft_batch(dev(smag), dev(sph), nfft=nfft))


def stream():
    model = build_model("FullyCNNV3", False, weights=_weights.synthetic_weights(3, seed=42))
    lanes = 5
    for nfft in (512, 256):
        rng = np.random.default_rng(nfft)
        s = audio.StreamingDenoiser(model, lanes, max_hops=8, nfft=nfft)
        step = [0]

        def push(k, active=None):
            pcm = (0.1 * rng.standard_normal((lanes, k * 128))).astype(np.float32)
            digest("stream%d/%02d_push%d" % (nfft, step[0], k), s.push(pcm, active))
            step[0] += 1

        def finish(which, tails):
            outs = s.finish(which, [(0.1 * rng.standard_normal(t)).astype(np.float32) for t in tails])
            assert all(len(o) > 0 for o in outs)
            digest("stream%d/%02d_finish%s" % (nfft, step[0], "".join(map(str, which))), np.concatenate(outs))
            OUT["stream%d/%02d_owed" % (nfft, step[0])] = [len(o) for o in outs]
            step[0] += 1

        push(1)
        finish([4], [127])                      # 1 hop pushed: frames 0 and 1 both come from the finish
        push(3, [1, 1, 1, 0, 1])                # lane 3 idle; lane 4 starts again
        finish([0], [0])                        # 4 hops: the head is still inside the finish
        push(8)
        finish([1], [1])
        push(3, [1, 0, 1, 1, 1])                # lane 1 idle
        push(1)
        finish([2, 3], [127, 0])
        push(8)                                 # every lane at another point of its utterance
        finish([0, 1, 2, 3, 4], [5, 0, 1, 127, 64])
        s.close()


def stoi():
    import stoi_np as sn
    lens = (65664, 24000, 24001, 30123, 9001, 6001, 13579, 65664)
    snrs = (5, 20, 10, 0, -5, 15, None, -5)
    clean = [sn.speechlike(n, 11 + i).astype(np.float32) for i, n in enumerate(lens)]
    est = [(c if q is None else sn.add_white(c.astype(np.float64), q, 111 + i)).astype(np.float32) for i, (c, q) in enumerate(zip(clean, snrs))]
    lens, clean, est = lens + (3000,), clean + [clean[0][:3000]], est + [est[0][:3000]]      # 3000 samples: under 30 spectral frames

    def padded(rows, width, fill):
        out = np.full((len(rows), width), fill, np.float32)
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
        return out

    for fs in (8000, 10000):
        d, det = audio.stoi_batch(dev(padded(clean, 65664 + 7, 7.0)), dev(padded(est, 65664 + 13, -3.0)), list(lens), sample_rate=fs, detail=True)
        digest("stoi/%d/scores" % fs, d)
        digest("stoi/%d/detail" % fs, det)
        OUT["stoi/%d/detail_values" % fs] = det.cpu().numpy().tolist()
        assert float(d[-1]) == 1e-5 and det[-1, 2].item() == 0 and det[0, 2].item() > 0


RATIOS = [(16000, 8000), (44100, 8000), (8000, 48000), (8000, 8000)]
FORMATS = [("int16", 2, "float32"), ("float32", 1, "int16")]


def pcm_of(rng, shape, dtype, channels):
    """seeded PCM of [.., frames] (+ [channels] when there are several) in a sample format"""
    shape = tuple(shape) + ((channels,) if channels > 1 else ())
    x = 0.3 * rng.standard_normal(shape)
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16) if dtype == "int16" else x.astype(np.float32)


def resample_offline(tag, rng, sr_in, sr_out, dtype, channels, out_dtype):
    import ctypes
    from fullycnnspeechenhancement_amd import _lib
    tile = ctypes.c_int()
    _lib.check(_lib.load().rced_rfree_plan(sr_in, sr_out, _lib.PCM_F32, 1, 64, 64, 0, None, ctypes.byref(tile), None, None))
    over = 0                                    # the fewest frames that give more than `tile` outputs: a second workgroup, all but idle
    while audio.resample_length(over, sr_in, sr_out) < tile.value + 1:
        over += 1
    lens = [0, 1, 777, over]
    OUT["%s/offline/lens" % tag] = [lens, tile.value]
    pcm = pcm_of(rng, (4, max(lens) + 5), dtype, channels)
    rows, out_lens = audio.resample_batch(dev(pcm), sr_in, sr_out, lengths=lens, dtype=out_dtype)
    assert out_lens[3] > tile.value >= audio.resample_length(over - 1, sr_in, sr_out)      # tile + 1 where the ratio gives that length
    digest("%s/offline/padded" % tag, rows)
    OUT["%s/offline/out_lens" % tag] = list(out_lens)
    arena = np.concatenate([pcm[i, :n] for i, n in enumerate(lens)] + [pcm[0, :3]])      # three frames of slack behind the rows
    begins = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    obegins = [2, 2, 3 + out_lens[1], 4 + out_lens[1] + out_lens[2]]      # row 0 is empty; a gap of one sample between the others
    out = torch.full((obegins[3] + out_lens[3] + 3,), 3, dtype=getattr(torch, out_dtype), device="cuda")
    packed, plens = audio.resample_arena(dev(arena), begins, lens, channels, sr_in, sr_out, out=out, out_begins=obegins, dtype=out_dtype)
    assert list(plens) == list(out_lens)
    digest("%s/offline/packed" % tag, packed)


def resample_units(tag, rng, sr_in, sr_out, dtype, channels, out_dtype):
    s = audio.StreamingResampler(sr_in, sr_out, 3, channels=channels, dtype=dtype, out_dtype=out_dtype, max_units=4)
    step = [0]

    def push(k, active=None):
        digest("%s/units/%02d_push%d" % (tag, step[0], k), s.push(pcm_of(rng, (3, k * s.unit_in), dtype, channels), active))
        digest("%s/units/%02d_started" % (tag, step[0]), s.started(active))
        step[0] += 1

    def finish(which, tails):
        outs = s.finish(which, [pcm_of(rng, (min(t, s.unit_in - 1),), dtype, channels) for t in tails])
        digest("%s/units/%02d_finish%s" % (tag, step[0], "".join(map(str, which))), np.concatenate(outs))
        OUT["%s/units/%02d_owed" % (tag, step[0])] = [len(o) for o in outs]
        step[0] += 1

    OUT["%s/units/geometry" % tag] = [s.unit_in, s.unit_out, s.delay, s.finish_max]
    push(1)
    push(4, [1, 0, 1])                      # lane 1 idle
    push(1)
    push(4, [0, 1, 1])                      # lane 0 idle
    finish([0, 1, 2], [0, 1, s.unit_in - 1])
    push(4)                                 # the lanes reused
    s.reset(1)
    push(1, [1, 1, 0])                      # lane 1 starts again, lane 2 idle
    finish([1], [1])
    push(4)
    s.reset()
    push(1)
    finish([2, 0], [s.unit_in - 1, 0])
    s.close()


def resample_free(tag, rng, sr_in, sr_out, dtype, channels, out_dtype, prefill):
    s = audio.FreeResampler(sr_in, sr_out, 3, channels=channels, dtype=dtype, out_dtype=out_dtype, max_frames=512, prefill=prefill)
    step = [0]

    def push(n, counts=None, take=None):
        out = s.push(pcm_of(rng, (3, n), dtype, channels) if n is not None else None, counts, take)
        digest("%s/free/%02d_push%s" % (tag, step[0], n), out)
        OUT["%s/free/%02d_taken" % (tag, step[0])] = [list(out.shape), [int(v) for v in s.taken], [int(v) for v in s.in_ring]]
        step[0] += 1

    def finish(which, tails):
        outs = s.finish(which, [pcm_of(rng, (t,), dtype, channels) for t in tails])
        digest("%s/free/%02d_finish%s" % (tag, step[0], "".join(map(str, which))), np.concatenate(outs))
        OUT["%s/free/%02d_owed" % (tag, step[0])] = [[len(o) for o in outs], [int(v) for v in s.owed], [int(v) for v in s.in_ring]]
        step[0] += 1

    OUT["%s/free/geometry" % tag] = [s.capacity, s.finish_max, s.max_take, s.prefill]
    push(441, take=0)
    push(None, take=[v // 2 for v in s.in_ring])      # a take alone, partial
    push(1)
    push(512, counts=[512, -1, 300])        # lane 1 idle, lane 2 given a part of its row
    push(0)
    push(1, take=0)
    finish([0, 1, 2], [700, 3, 0])          # lane 0's tail goes through a push first
    push(441, counts=[-1, 441, 441])        # the lanes reused
    s.reset(1)
    push(512)
    s.reset()
    push(1)
    finish([2], [1])
    s.close()


def resample_chains():
    model = build_model("FullyCNNV3", False, weights=_weights.synthetic_weights(3, seed=42))
    rng = np.random.default_rng(77)
    s = audio.StreamingDenoiser(model, 2, max_hops=4, sample_rate=16000, output_rate=16000, dtype="int16")
    OUT["resample/chain/stream_geometry"] = [s.hop, s.hop_in, s.delay]
    for i, (k, active) in enumerate([(1, None), (4, [1, 0]), (2, None)]):
        digest("resample/chain/stream_push%d" % i, s.push(pcm_of(rng, (2, k * s.hop_in), "int16", 1), active))
    outs = s.finish([0, 1], [pcm_of(rng, (t,), "int16", 1) for t in (s.hop_in - 1, 0)])
    digest("resample/chain/stream_finish", np.concatenate(outs))
    s.reset()
    digest("resample/chain/stream_again", s.push(pcm_of(rng, (2, s.hop_in), "int16", 1)))
    s.close()
    b = audio.BlockDenoiser(model, 2, 441, sample_rate=44100)
    OUT["resample/chain/block_geometry"] = [b.block_out, b.prefill, b.delay, list(b.hops_per_call)]
    for i, active in enumerate([None, [1, 0], None, None, [0, 1], None]):
        digest("resample/chain/block_call%d" % i, b.process(pcm_of(rng, (2, 441), "float32", 1), active))
    outs = b.finish([0, 1], [pcm_of(rng, (t,), "float32", 1) for t in (440, 0)])
    digest("resample/chain/block_finish", np.concatenate(outs))
    b.reset(0)
    digest("resample/chain/block_again", b.process(pcm_of(rng, (2, 441), "float32", 1)))
    b.close()


def resample():
    for sr_in, sr_out in RATIOS:
        for i, (dtype, channels, out_dtype) in enumerate(FORMATS):
            tag = "resample/%d_%d/%s" % (sr_in, sr_out, dtype)
            rng = np.random.default_rng(sr_in + sr_out + i)
            resample_offline(tag, rng, sr_in, sr_out, dtype, channels, out_dtype)
            resample_units(tag, rng, sr_in, sr_out, dtype, channels, out_dtype)
            resample_free(tag, rng, sr_in, sr_out, dtype, channels, out_dtype, prefill=7 if (sr_in, i) == (44100, 0) else 0)
    resample_chains()


if __name__ == "__main__":
    sections = (stft_istft, stream, stoi, resample)
    unknown = set(sys.argv[1:]) - set(s.__name__ for s in sections)
    if unknown:
        sys.exit("no such section: %s (there are: %s)" % (", ".join(sorted(unknown)), ", ".join(s.__name__ for s in sections)))
    for section in sections:
        if len(sys.argv) < 2 or section.__name__ in sys.argv[1:]:
            section()
    torch.cuda.synchronize()
    print(json.dumps(OUT, sort_keys=True))
