"""Writes tests/golden/ctc_beam_parent_bits.npz: the inputs of the cases of tests/test_ctc_beam_parent_bits_gpu.py and every
output of the library AS BUILT on them, with the commit that library was built from (run once, on a GPU, with the library whose bits
are to be kept; the file is committed):  python tools/make_ctc_beam_fixture.py --commit $(git rev-parse HEAD)

Cases, calls and the model's word list are the test's own (CASES, MODES, WORDS, `decode`); the inputs are drawn here, once, and
stored.  The seed of the pruned case is one where a row of the float64 restatement (tests/_ctc_beam_ref.py) has a prefix that comes
back into the beam beside a live child; that is checked before anything is written."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ctc_beam_ref as B  # noqa: E402
import test_ctc_beam_parent_bits_gpu as T  # noqa: E402

PRUNED_SEED, PRUNED_SHARP = 5, 1.5


def inputs():
    """{stored name: array [N, T, C]}"""
    pruned = B.posterior(np.random.RandomState(PRUNED_SEED), 5, 12, 12, PRUNED_SHARP)
    assert any(r['reentries'] > 0 for r in B.decode(B.logs(pruned), 8, 3, 6)), "no row of the pruned case has a re-entry"
    dead = pruned.copy()
    dead[T.DEAD, 7, :] = 0.0
    dead[T.DEAD, 7, 1] = 1.0
    return {
        "pruned": pruned,
        "pruned_bf16": torch.from_numpy(pruned).to(torch.bfloat16).view(torch.int16).numpy(),
        "pruned_logs": B.logs(pruned),
        "full": B.posterior(np.random.RandomState(70), 2, 4, 70, 2.0),
        "smallest": B.posterior(np.random.RandomState(1), 1, 1, 12, 1.0),
        "dead_row": dead,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ctc_beam_parent_bits.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("make_ctc_beam_fixture.py records what the GPU computes; there is none")
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
    assert len(commit) == 40, commit
    stored = inputs()
    stored["parent_commit"] = np.array(commit)
    lm = T.model()
    for case in sorted(T.CASES):
        for mode in sorted(T.MODES):
            out = T.decode(stored, case, mode, lm)
            for key, value in out.items():
                stored["%s.%s.%s" % (case, mode, key)] = value
            print("%-12s %-8s count %s" % (case, mode, out['count'].tolist()))
    dead = stored["dead_row.plain.count"]
    assert dead[T.DEAD] == 0 and np.all(np.delete(dead, T.DEAD) > 0), dead
    assert np.all(stored["full.plain.count"] == 64), "the full case does not fill the beam"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **stored)
    print("%s: %d arrays, %d bytes" % (args.out, len(stored), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
