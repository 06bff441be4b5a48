#!/usr/bin/env python3
"""Generate tests/golden/classify/cases.json by IMPORTING the reference (build machine only; no test runs this).

For every case the reference's own functions (``construct_graph``, ``find_initial_cliques``,
``find_cliques_recursively``, ``get_unique_cliques``, ``compute_classify_output``; pyani_plus/classify.py and the
call sequence of public_cli.py:1299-1330) run in child processes under several ``PYTHONHASHSEED`` values, because the
reference hands sets of strings around and its row and member order -- and, with tied scores, its rows -- change with
the hash seed.  Two conditions are asserted for every case that is kept:

* no two edges have the same score (``-0.0`` and ``0.0`` count as the same);
* the rows, as a map from member set to values, are the same under every hash seed.

A generated case that fails either is tried again with the next seed, not kept.  Stored per case: the settings that
rebuild the input (tests/classify_cases.py), an md5 of the rebuilt matrices and of the score matrix handed to the
reference, and the reference's rows sorted by sorted members: the raw values as ``repr`` and the text fields of its TSV.

    python tests/golden/classify/make_classify_golden.py      # needs /root/reference and networkx
"""

from __future__ import annotations

import contextlib
import io
import json
import math
import os
import subprocess
import sys
import tempfile
from pathlib import Path

REFERENCE = Path("/root/reference")
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent.parent
HASH_SEEDS = ("0", "1", "2")
AGGS = ("min", "max", "mean")


def case_specs() -> list[dict]:
    """The cases without their results (the seed of a generated one may be moved on by ``main``)."""
    specs = []

    def add(name, source, *, mode="identity", coverage_edges="min", score_edges="mean", cov_min=0.5):
        specs.append({"name": name, "source": source, "mode": mode, "coverage_edges": coverage_edges, "score_edges": score_edges,
                      "cov_min": cov_min})

    for fixture, methods in (("viral_example", ("fastANI", "sourmash")), ("bacterial_example", ("fastANI", "sourmash")), ("bad_alignments", ("sourmash",))):
        for method in methods:
            for mode in ("identity", "tANI"):
                for cov_min in (0.0, 0.5):
                    add(f"{fixture}-{method}-{mode}-cov{cov_min}", {"fixture": fixture, "method": method}, mode=mode, cov_min=cov_min)

    def synth(n, seed, **kw):
        return {"synth": {"n": n, "seed": seed, **kw}}

    # group structure at every size; cross-species coverage straddles the threshold
    for n in (1, 2, 3, 16, 60, 200):
        add(f"synth-n{n}", synth(n, 1))
    add("synth-n60-tani", synth(60, 2), mode="tANI")
    add("synth-n60-complete", synth(60, 3, groups=2), cov_min=0.1)
    # 5 % NaN cells, placed per direction
    for n in (3, 16, 60):
        add(f"synth-n{n}-nan", synth(n, 4, nan_frac=0.05))
    add("synth-n16-nan-tani", synth(16, 5, nan_frac=0.05), mode="tANI", coverage_edges="max", score_edges="min")
    # every aggregator in both roles, with NaN cells so that the argument order of min and max matters
    for ca in AGGS:
        for sa in AGGS:
            add(f"synth-n16-agg-{ca}-{sa}", synth(16, 6, nan_frac=0.05), coverage_edges=ca, score_edges=sa)
    # disconnected from the start
    add("synth-n30-disconnected", synth(30, 7, cross_cov=0.2))
    add("synth-n30-disconnected-nan", synth(30, 8, cross_cov=0.2, nan_frac=0.05))
    add("synth-n16-no-edge", synth(16, 9), cov_min=1.0)
    add("synth-n2-no-edge", synth(2, 9), cov_min=1.0)
    add("synth-n24-lowest-edge-in-clique", synth(24, 10, cross_cov=0.2, low_group=True, subgroups=1))
    # the thresholds
    for cov_min in (0.0, 0.5, 1.0):
        add(f"synth-n30-cov{cov_min}", synth(30, 11), cov_min=cov_min)
    return specs


def reference_input(spec: dict):
    """(labels, coverage frame, score frame handed to construct_graph, base identity, base coverage)."""
    import numpy as np
    import pandas as pd

    sys.path.insert(0, str(ROOT))
    from tests.classify_cases import base_matrices

    labels, ident, cov = base_matrices(spec["source"])
    cov_frame = pd.DataFrame(cov, index=labels, columns=labels)
    if spec["mode"] == "identity":
        score_frame = pd.DataFrame(ident, index=labels, columns=labels)
    else:
        hadamard = pd.DataFrame(ident * cov, index=labels, columns=labels)
        tani = hadamard.map(lambda x: -math.log(x) if x else np.nan, na_action="ignore")  # db_orm.py:588
        score_frame = tani.where(tani.isna(), tani * -1)  # public_cli.py:1269
    return labels, cov_frame, score_frame, ident, cov


def child(spec_file: str) -> None:
    """Run the reference on every spec of the file; print one JSON list of per-case results."""
    sys.path.insert(0, str(ROOT))
    import tests.classify_cases  # noqa: F401  (this repository's tests package, before the reference's is on the path)

    sys.path.append(str(REFERENCE))
    import networkx as nx
    from pyani_plus import classify

    results = []
    for spec in json.loads(Path(spec_file).read_text()):
        _labels, cov, score, _i, _c = reference_input(spec)
        graph = classify.construct_graph(cov, score, classify.AGG_FUNCS[spec["coverage_edges"]], classify.AGG_FUNCS[spec["score_edges"]], spec["cov_min"])
        scores = sorted(a["score"] + 0.0 for _, _, a in graph.edges(data=True))
        tied = any(x == y for x, y in zip(scores, scores[1:]))
        components, n_edges = len(list(nx.connected_components(graph))), graph.number_of_edges()  # the recursion removes edges
        initial = classify.find_initial_cliques(graph) if components != 1 else []
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            recursive = classify.find_cliques_recursively(graph)
        unique = classify.get_unique_cliques(initial, recursive)
        suffix = "identity" if spec["mode"] == "identity" else "-tANI"
        with tempfile.TemporaryDirectory() as tmp:
            info, _frame = classify.compute_classify_output(unique, "golden", Path(tmp), {"min_score": f"min_{suffix}", "max_score": f"max_{suffix}"})
            lines = (Path(tmp) / "golden_classify.tsv").read_text().split("\n")
        assert lines[-1] == "" and len(lines) == len(info) + 2
        rows = []
        for clique, line in zip(info, lines[1:]):
            fields = line.split("\t")
            assert sorted(fields[4].split(",")) == sorted(clique.members)
            rows.append({
                "members": sorted(clique.members),
                "raw": [clique.n_nodes] + [None if v is None else repr(float(v)) for v in (clique.max_cov, clique.min_score, clique.max_score)],
                "tsv": fields[:4],
            })  # fmt: skip
        rows.sort(key=lambda r: r["members"])
        results.append({"header": lines[0], "n_edges": n_edges, "components": components, "tied": tied, "rows": rows})
    print(json.dumps(results))


def run_children(specs: list[dict]) -> list[list[dict]]:
    with tempfile.TemporaryDirectory() as tmp:
        spec_file = Path(tmp) / "specs.json"
        spec_file.write_text(json.dumps(specs))
        out = []
        for seed in HASH_SEEDS:
            env = dict(os.environ, PYTHONHASHSEED=seed, PYTHONDONTWRITEBYTECODE="1")
            done = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", str(spec_file)], env=env, capture_output=True, text=True, check=False)
            if done.returncode != 0:
                raise SystemExit(f"child under PYTHONHASHSEED={seed} failed:\n{done.stderr[-3000:]}")
            out.append(json.loads(done.stdout.strip().split("\n")[-1]))
        return out


def main() -> None:
    if not REFERENCE.is_dir():
        raise SystemExit("the reference checkout is needed to regenerate these vectors")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ROOT))
    from tests.classify_cases import matrices_md5

    pending = case_specs()
    kept: dict[str, dict] = {}
    for attempt in range(6):
        if not pending:
            break
        per_seed = run_children(pending)
        again = []
        for k, spec in enumerate(pending):
            results = [r[k] for r in per_seed]
            stable = all(r["rows"] == results[0]["rows"] and r["header"] == results[0]["header"] for r in results)
            if results[0]["tied"] or not stable:
                why = "tied scores" if results[0]["tied"] else "rows differ between hash seeds"
                if "synth" not in spec["source"]:
                    raise SystemExit(f"fixture case {spec['name']}: {why}")
                print(f"{spec['name']}: {why} with seed {spec['source']['synth']['seed']}, trying the next seed", file=sys.stderr)
                spec["source"]["synth"]["seed"] += 100
                again.append(spec)
                continue
            _labels, _cov, score, ident, cov = reference_input(spec)
            kept[spec["name"]] = {**spec, "md5": matrices_md5(ident, cov), "score_md5": matrices_md5(score.to_numpy(dtype=float)),
                                  **{key: results[0][key] for key in ("header", "n_edges", "components", "rows")}}
        pending = again
    if pending:
        raise SystemExit(f"no untied, stable input found for {[s['name'] for s in pending]}")
    order = [s["name"] for s in case_specs()]
    cases = [kept[name] for name in order]
    assert any(c["components"] > 1 and c["n_edges"] == 0 for c in cases) and any(c["components"] > 1 and c["n_edges"] > 0 for c in cases)
    # one case per line; a row is [members joined by commas, raw, tsv] (tests/classify_cases.py::load_cases undoes it)
    for case in cases:
        case["rows"] = [[",".join(r["members"]), r["raw"], r["tsv"]] for r in case["rows"]]
    lines = ",\n".join(json.dumps(case, separators=(",", ":")) for case in cases)
    (HERE / "cases.json").write_text('{"hash_seeds":' + json.dumps(list(HASH_SEEDS)) + ',"cases":[\n' + lines + "\n]}\n")
    print(f"wrote {len(cases)} cases to {HERE / 'cases.json'}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
