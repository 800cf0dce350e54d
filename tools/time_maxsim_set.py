"""Time `set_multivec` on one GPU next to the rebuild it replaces (close the index, `add_multivec` the whole store from the host).

    python tools/time_maxsim_set.py --docs 100000 --tokens 100 --dim 128 --repeats 5

Calls timed (host clock around calls that are complete on return), median and range over `--repeats`:
  a  an in-place set of 1 document            b  an in-place set of 1 % of the documents
  c  a relayout set of 1 document             d  a removal of 1 % of the documents (followed, untimed, by their revival)
  rebuild  a new index + add_multivec of the whole store from host memory
Prints one JSON line.  Document lengths are drawn from [tokens - 20, tokens + 20]; an in-place set keeps each listed document's
length, a relayout set adds 32 tokens to it."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    lens = rng.integers(max(1, a.tokens - 20), a.tokens + 21, size=a.docs).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = rng.standard_normal((int(off[-1]), a.dim), dtype=np.float32)

    def payload(ids, new_lens):
        o = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.int64)
        return ids, rng.standard_normal((int(o[-1]), a.dim), dtype=np.float32), o

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def rebuild():
        with Mi355Index(a.dim) as fresh:
            fresh.add_multivec(tok, off)
            fresh.synchronize()

    times: dict[str, list[float]] = {key: [] for key in ("a", "b", "c", "d", "rebuild")}
    cur = lens.copy()
    one_pct = max(1, a.docs // 100)
    with Mi355Index(a.dim) as idx:
        idx.add_multivec(tok, off)
        idx.set_multivec(*payload(np.array([0]), cur[[0]]))                    # warm-up of both paths (code objects, allocator)
        idx.set_multivec(*payload(np.array([1]), cur[[1]] + 32))
        cur[1] += 32
        rebuild()
        for _ in range(a.repeats):
            i = rng.choice(a.docs, 1)
            p = payload(i, cur[i])
            times["a"].append(timed(lambda: idx.set_multivec(*p)))
            ids = np.sort(rng.choice(a.docs, one_pct, replace=False))
            p = payload(ids, cur[ids])
            times["b"].append(timed(lambda: idx.set_multivec(*p)))
            i = rng.choice(a.docs, 1)
            p = payload(i, cur[i] + 32)
            times["c"].append(timed(lambda: idx.set_multivec(*p)))
            cur[i] += 32
            ids = np.sort(rng.choice(a.docs, one_pct, replace=False))
            times["d"].append(timed(lambda: idx.remove_multivec(ids)))
            idx.set_multivec(*payload(ids, cur[ids]))                          # (revived, untimed: the store keeps its size)
            times["rebuild"].append(timed(rebuild))
        moved, set_docs = idx.stat("maxsim_moved_blocks"), idx.stat("maxsim_set_docs")
    blocks = int(((lens + 31) // 32).sum())
    out = {"docs": a.docs, "token_vectors": int(off[-1]), "dim": a.dim, "blocks": blocks,
           "image_bytes": blocks * 32 * a.dim * 6, "repeats": a.repeats, "moved_blocks": moved, "set_docs": set_docs,
           "ms": {key: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                  for key, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
