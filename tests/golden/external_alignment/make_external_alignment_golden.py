"""Generate the external-alignment golden vectors by IMPORTING the reference (this container only).

For seeded alignments every subject column is computed by the reference's own ``compute_external_alignment_column``
and its rows are stored in the order it yields them.  The alignments themselves are not stored: each entry keeps the
generator settings (``tests/msa_checker.golden_msa_bytes``: IUPAC codes, lower case, '.', gap and N runs, an all-gap
column, mixed line widths and '\\r\\n') and the md5 of the text, which the tests check before they compare.  A row is
``[query index, subject index, identity, aln_length, sim_errors, cov_query, cov_subject]``, indices into ``hashes``
(the record names, which the ``md5`` label maps to themselves); one line per column.

    python tests/golden/external_alignment/make_external_alignment_golden.py      # needs the reference checkout
"""

from __future__ import annotations

import datetime
import hashlib
import json
import logging
import sys
import tempfile
from pathlib import Path

REFERENCE = Path("/root/reference")
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent.parent

# the reference's expected matrices for its 3 x 11 mock (tests/test_external_alignment.py of the reference)
_H = '["5584c7029328dc48d33f95f0a78f7e57","689d3fd6881db36b5e08329cf23cecdd","78975d5144a1cd12e98898d573cf6536"]'
MOCK_DF_IDENTITY = '{"columns":' + _H + ',"index":' + _H + ',"data":[[1.0,0.8,0.8],[0.8,1.0,0.9],[0.8,0.9,1.0]]}'
MOCK_DF_COV_QUERY = '{"columns":' + _H + ',"index":' + _H + ',"data":[[1.0,0.9,1.0],[1.0,1.0,1.0],[1.0,0.9,1.0]]}'
SEEDED = {
    "seeded_dna": {"rows": 12, "columns": 4000, "seed": 11, "prefix": "d", "opts": {"divergence": 0.03, "gap_runs": 5e-4, "n_runs": 2e-4}},
    "seeded_iupac": {"rows": 12, "columns": 4000, "seed": 12, "prefix": "i",
                     "opts": {"divergence": 0.05, "gap_runs": 5e-4, "n_runs": 2e-4, "iupac": 0.01, "lower": 0.02, "dots": 0.005}},
    "seeded_divergent": {"rows": 10, "columns": 1500, "seed": 13, "prefix": "v",
                         "opts": {"divergence": 0.2, "gap_runs": 2e-3, "iupac": 0.02, "lower": 0.05}},
}


def main() -> None:
    if not REFERENCE.is_dir():
        raise SystemExit("the reference checkout is needed to regenerate these vectors")
    sys.dont_write_bytecode = True
    if not hasattr(datetime, "UTC"):
        datetime.UTC = datetime.timezone.utc
    sys.path.insert(0, str(REFERENCE))
    sys.path.insert(0, str(ROOT))
    from pyani_plus.methods.external_alignment import compute_external_alignment_column

    import importlib.util  # the reference's own tests/ package would shadow ours

    spec_ = importlib.util.spec_from_file_location("msa_checker", ROOT / "tests" / "msa_checker.py")
    checker = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(checker)
    golden_msa_bytes = checker.golden_msa_bytes

    logger = logging.getLogger("golden")
    lines = ["{", '"provenance": "tests/golden/external_alignment/make_external_alignment_golden.py, from the reference",',
             f'"mock": {json.dumps({"file": "mock_3x11.fasta", "df_identity": MOCK_DF_IDENTITY, "df_cov_query": MOCK_DF_COV_QUERY})},',
             '"msas": {']
    for k, (name, spec) in enumerate(SEEDED.items()):
        text = golden_msa_bytes(spec)
        hashes = sorted(f"{spec['prefix']}{i:02d}" for i in range(spec["rows"]))
        index = {h: i for i, h in enumerate(hashes)}
        with tempfile.TemporaryDirectory() as tmp:
            path = Path(tmp) / f"{name}.fasta"
            path.write_bytes(text)
            columns = [[[index[r[0]], index[r[1]], *r[2:]] for r in
                        compute_external_alignment_column(logger, s, set(hashes), path, lambda x: x, "md5")] for s in hashes]  # fmt: skip
        head = {"spec": spec, "md5": hashlib.md5(text).hexdigest(), "hashes": hashes}
        lines.append(f'{json.dumps(name)}: {json.dumps(head)[:-1]}, "columns": [')
        lines.extend(json.dumps(c, separators=(",", ":")) + ("," if i + 1 < len(columns) else "") for i, c in enumerate(columns))
        lines.append("]}" + ("," if k + 1 < len(SEEDED) else ""))
    lines += ["}", "}"]
    (HERE / "columns.json").write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
