#!/usr/bin/env python3
"""Brings a corpus of PCM16 wav files to one sample rate on the GPU and writes the reference's manifest for it: what
Work/datasets/*_prepare.py do after unpacking (resampy.resample(.., filter='kaiser_best') file by file on the CPU, then json
lines {audio_filepath, duration}), with the conversion of DESIGN.md 3.4f.

    python tools/prepare_corpus.py SOURCE OUT_ROOT MANIFEST [--sample-rate 8000] [--device 0]

SOURCE: a directory (every *.wav under it, sorted) or a manifest (its audio_filepath entries).  Every file is downmixed,
resampled and written as mono PCM16 (clip(rint(y * 32768))) under OUT_ROOT at its path relative to SOURCE (for a manifest:
relative to the files' common directory); a file already mono at the rate is copied through the same path, sample for
sample.  Files of fewer than 100 frames are skipped, as the reference's scripts skip them.  duration = samples / rate of
the written file.  Needs a GPU; there is no CPU fallback.  Prints one JSON line: files, skipped, seconds of audio, wall time."""
import argparse, codecs, json, os, sys, time, wave
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

MIN_FRAMES = 100


def list_sources(source):
    """(paths, base): the wav files and the directory their output paths are relative to."""
    if os.path.isdir(source):
        paths = sorted(os.path.join(d, f) for d, _, files in os.walk(source) for f in files if f.lower().endswith(".wav"))
        return paths, source
    paths = [json.loads(line)["audio_filepath"] for line in codecs.open(source, "r", "utf-8") if line.strip()]
    return paths, (os.path.commonpath([os.path.dirname(os.path.abspath(p)) for p in paths]) if paths else ".")


def prepare(source, out_root, manifest, sample_rate=8000, device=0):
    from fullycnnspeechenhancement_amd import audio, loader
    import torch
    t0 = time.perf_counter()
    paths, base = list_sources(source)
    kept = [p for p in paths if loader.wav_info(p)[2] >= MIN_FRAMES]
    lines, seconds = [None] * len(kept), 0.0
    for raw, groups in loader.staged_uploads(kept, "cuda:%d" % device):
        for (rate, channels), rows in groups.items():
            lens = [audio.resample_length(f, rate, sample_rate) for _, _, f in rows]
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            out = torch.empty((int(offs[-1]),), dtype=torch.int16, device=raw.device)
            audio.resample_arena(raw, [a for _, a, _ in rows], [f for _, _, f in rows], channels, rate, sample_rate, out=out,
                                 out_begins=offs[:-1].tolist(), dtype="int16")
            pcm = out.cpu().numpy()
            for (i, _, _), off, n in zip(rows, offs, lens):
                dst = os.path.join(out_root, os.path.relpath(os.path.abspath(kept[i]), os.path.abspath(base)))
                os.makedirs(os.path.dirname(dst), exist_ok=True)
                w = wave.open(dst, "wb")
                try:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(sample_rate)
                    w.writeframes(pcm[off:off + n].astype("<i2").tobytes())
                finally:
                    w.close()
                lines[i] = json.dumps({"audio_filepath": dst, "duration": float(n) / sample_rate}, ensure_ascii=False)
                seconds += float(n) / sample_rate
    if os.path.dirname(manifest):
        os.makedirs(os.path.dirname(manifest), exist_ok=True)
    with codecs.open(manifest, "w", "utf-8") as fout:
        for line in lines:
            fout.write(line + "\n")
    return {"files": len(kept), "skipped": len(paths) - len(kept), "audio_s": seconds, "wall_s": time.perf_counter() - t0}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source")
    ap.add_argument("out_root")
    ap.add_argument("manifest")
    ap.add_argument("--sample-rate", type=int, default=8000)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    print(json.dumps(prepare(a.source, a.out_root, a.manifest, a.sample_rate, a.device)))
