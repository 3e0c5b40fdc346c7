"""One RELOC query of the device KeyFrameDatabase at 1000 and 4000 key frames of ~1500 words: median of event-bracketed
repetitions after warm-up (every repetition uses a fresh query id, so every one lists and scores).  The Python restatement
(tests/kfdb_ref.py) is timed on the same inputs for scale; a compiled CPU twin does not exist yet.

    python profiles/probes/kfdb_probe.py profiles/kfdb_probe.json
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kfdb_ref as R  # noqa: E402
from fishbirdeyevisualslam_amd import kfdb_problem as P  # noqa: E402
from fishbirdeyevisualslam_amd.kfdb import KeyFrameDatabase  # noqa: E402


def main(out):
    res = {"what": "one DetectRelocalizationCandidates query, ~1500 words per BowVector", "reps": 30, "warmup": 5, "cases": []}
    for n_kf in (1000, 4000):
        p = P.make_random_database(31 + n_kf, n_kf, words=(1400, 1600), vocab=100000)
        dev = KeyFrameDatabase(4096, 2048)
        dev.set_covisibility(np.concatenate([p["covis"], np.full((4096 - n_kf, 10), -1, np.int32)]))
        for s, (ids, vals) in enumerate(p["bows"]):
            dev.add(s, ids, vals)
        ids, vals = p["bows"][7]
        torch.cuda.synchronize()
        times = []
        for rep in range(35):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n, di, dv = dev._bow(None, ids, vals)
            a.record()
            got = dev.detect_relocalization_candidates(1000 + rep, di, dv, n_words=n, extras=True)
            b.record()
            torch.cuda.synchronize()
            if rep >= 5:
                times.append(a.elapsed_time(b))
        ref = R.KeyFrameDatabase(4096)
        for s, (i2, v2) in enumerate(p["bows"]):
            ref.add(s, i2, v2)
        t0 = time.perf_counter()
        want = ref.detect_relocalization_candidates(1, ids, vals, p["covis"])
        t_py = time.perf_counter() - t0
        case = dict(n_keyframes=n_kf, gpu_ms_median=float(np.median(times)), gpu_ms_min=float(np.min(times)), gpu_ms_max=float(np.max(times)),
                    n_sharing=int(got["n_sharing"].cpu()[0]), n_scored=int(got["n_scored"].cpu()[0]),
                    n_candidates=int(got["n_candidates"].cpu()[0]), python_restatement_ms=1e3 * t_py, compiled_cpu_restatement_ms="not measured",
                    same_counts_as_restatement=bool(int(got["n_sharing"].cpu()[0]) == want["n_sharing"] and int(got["n_scored"].cpu()[0]) == want["n_scored"]))
        print(case, flush=True)
        res["cases"].append(case)
        dev.close()
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "kfdb_probe.json")
