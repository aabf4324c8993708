#!/usr/bin/env python3
"""Generate the fixtures that let tests/test_oracle_golden.py pin the oracle to the reference on a checkout that has
neither the reference tree nor oracle/_ref (dev container only; needs oracle/_ref/libspeexref.so built):

  * resources/<file>           the first EXCERPT_BYTES bytes of each of the reference's resources/*.pcm, read raw
                               as the reference's own test reads them (header bytes included)
  * golden_resources.json      per resources row of golden.json: output frames and sha1 of the reference's native C
                               run over that excerpt in one call sequence ("whole")
  * golden_random_configs.json the reference's results on the 40 random configurations of
                               test_oracle_equals_reference_build_on_random_configs (table, counters, positions,
                               output and history digests of every call: run_random_trial) and on the 25 random
                               control scripts of test_oracle_equals_reference_build_on_random_control_scripts (every
                               op's row, output, history and pending-frame digests: run_control_script), one
                               record_digest per trial

What is stored is DATA only: short excerpts, parameters, counters and sha1 digests.
Run:  python tests/golden/make_golden_standalone.py [REFERENCE_TREE]
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle as orc  # noqa: E402
from golden_util import drive, sha1  # noqa: E402

EXCERPT_BYTES = 1 << 16
RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000]


def record_digest(record):
    """sha1 of a trial's record (run_random_trial / run_control_script) in canonical JSON"""
    return hashlib.sha1(json.dumps(record, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def random_config_trials():
    """The trial sequence of test_oracle_equals_reference_build_on_random_configs: (ch, in, out, q, calls), calls =
    [(frames, capacity, seed)]."""
    rng = np.random.RandomState(1)
    trials = []
    for trial in range(40):
        ch = int(rng.randint(1, 5))
        i, o = int(rng.choice(RATES)), int(rng.choice(RATES))
        q = int(rng.randint(0, 11))
        calls = []
        for call in range(4):
            f = int(rng.choice([0, 1, 100, 777, 3000]))
            cap = int(rng.choice([0, 10, 1000, 100000]))
            calls.append((f, cap, trial * 10 + call))
        trials.append((ch, i, o, q, calls))
    return trials


def run_random_trial(engine_cls, ch, i, o, q, calls):
    """One trial on `engine_cls` (orc.Oracle or orc.Reference): the digests the golden file stores."""
    e = engine_cls(ch, i, o, q)
    row = {"channels": ch, "in_rate": i, "out_rate": o, "quality": q,
           "table_sha1": sha1(e.table().view(np.uint32)), "calls": []}
    for f, cap, seed in calls:
        x = orc.lcg_pcm(f * ch, seed).reshape(f, ch)
        out, used = e.process(x, cap)
        row["calls"].append({"frames": f, "capacity": cap, "seed": seed, "used": int(used),
                             "out_frames": int(out.shape[0]), "out_sha1": sha1(out),
                             "position": [int(v) for v in e.position()],
                             "history_sha1": [sha1(e.history(c)) for c in range(ch)]})
    return row


def random_control_scripts():
    """The scripts of test_oracle_equals_reference_build_on_random_control_scripts: (args, ops) per seed."""
    scripts = []
    for seed in range(25):
        r = np.random.RandomState(seed)
        ch = int(r.choice([1, 2, 5]))
        args = (ch, int(r.choice([8000, 11025, 44100, 48000])), int(r.choice([8000, 16000, 48000])),
                int(r.randint(0, 11)))
        ops = []
        for _ in range(20):
            pick = r.randint(0, 6)
            if pick < 3:
                op = ["int" if r.rand() < 0.5 else "float", int(r.randint(0, 1500)), int(r.randint(0, 3000)),
                      int(r.randint(1, 1 << 30))]
            elif pick == 3:
                op = ["rate", int(r.choice([8000, 11025, 44100, 48000])), int(r.choice([8000, 16000, 48000]))]
            elif pick == 4:
                op = ["quality", int(r.randint(0, 11))]
            else:
                op = [["skip"], ["reset"]][int(r.randint(0, 2))]
            ops.append(op)
        scripts.append((args, ops))
    return scripts


def run_control_script(engine_cls, args, ops):
    """One control script on `engine_cls`: per op [row, output sha1 or None, history sha1s, pending sha1s]."""
    from make_golden import apply_op
    e, rows = engine_cls(*args), []
    for op in ops:
        row, y = apply_op(e, op, args[0])
        rows.append([row, None if y is None else sha1(y),
                     [sha1(e.history(c)) for c in range(args[0])], [sha1(e.pending(c)) for c in range(args[0])]])
    return {"args": list(args), "ops": ops, "rows": rows}


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE", "")
    res_dir = os.path.join(ref_root, "resources")
    if not orc.have_reference() or not os.path.isdir(res_dir):
        sys.exit("make_golden_standalone.py: needs oracle/_ref built and REFERENCE_TREE/resources")
    golden = json.load(open(os.path.join(HERE, "golden.json")))
    out_dir = os.path.join(HERE, "resources")
    os.makedirs(out_dir, exist_ok=True)
    files, cases = {}, []
    for r in golden["resources"]:
        if r["file"] not in files:
            raw = np.fromfile(os.path.join(res_dir, r["file"]), dtype=np.uint8)[:EXCERPT_BYTES]
            raw.tofile(os.path.join(out_dir, r["file"]))
            files[r["file"]] = sha1(raw)
        raw = np.fromfile(os.path.join(out_dir, r["file"]), dtype=np.uint8)
        raw = raw[: raw.size - raw.size % (2 * r["channels"])]
        x = raw.view(np.int16).reshape(-1, r["channels"])
        spec = dict(channels=r["channels"], in_rate=r["in_rate"], out_rate=r["out_rate"], chunks="whole")
        want, _ = drive(orc.Reference(r["channels"], r["in_rate"], r["out_rate"], r["quality"]), spec, x)
        got, _ = drive(orc.Oracle(r["channels"], r["in_rate"], r["out_rate"], r["quality"]), spec, x)
        assert np.array_equal(want, got), r
        cases.append({k: r[k] for k in ("file", "channels", "in_rate", "out_rate", "quality")} |
                     {"in_frames": int(x.shape[0]), "out_frames": int(want.shape[0]), "sha1": sha1(want)})
    with open(os.path.join(HERE, "golden_resources.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_standalone.py (oracle/_ref: the reference's native C)",
                   "excerpt_bytes": EXCERPT_BYTES, "files": files, "cases": cases}, f, indent=1)
        f.write("\n")
    trials = [record_digest(run_random_trial(orc.Reference, *t)) for t in random_config_trials()]
    scripts = [record_digest(run_control_script(orc.Reference, *c)) for c in random_control_scripts()]
    with open(os.path.join(HERE, "golden_random_configs.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_standalone.py (oracle/_ref: the reference's native C)",
                   "digest": "record_digest: sha1 of each trial's record in canonical JSON",
                   "trials": trials, "control_scripts": scripts}, f, indent=1)
        f.write("\n")
    print("wrote %d excerpt(s), %d resource case(s), %d random-config trial(s)" % (len(files), len(cases), len(trials)))


if __name__ == "__main__":
    main()
