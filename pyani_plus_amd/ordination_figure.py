"""The figure of ordinate-run, drawn with matplotlib alone: the genomes as points, PC1 against PC2 (with one axis only,
PC1 against zero), each axis labelled with its proportion of the trace.  The reference has no such figure; the layout is
this project's own.  Everything is drawn from what ``ordination.pcoa`` returned.  matplotlib is imported when the first
figure is drawn."""

from __future__ import annotations

from pathlib import Path

import numpy as np

from . import ordination

POINT = "#2678B2"
MAX_LABELLED = 40  # genomes: beyond this the labels would cover the points


def axis_label(result: ordination.Ordination, c: int) -> str:
    return f"PC{c + 1} ({100.0 * float(result.proportions[c]):.1f}% of trace)"


def ordination_figure(result: ordination.Ordination, labels, name: str):
    """The figure of the ordination ``name``; the caller closes it."""
    import matplotlib as mpl

    mpl.use("agg")  # non-interactive backend
    import matplotlib.pyplot as plt

    figure, ax = plt.subplots(figsize=(8, 8))
    try:
        x = result.coordinates[:, 0]
        two = result.coordinates.shape[1] > 1
        y = result.coordinates[:, 1] if two else np.zeros_like(x)
        ax.scatter(x, y, s=18, color=POINT, alpha=0.8, linewidths=0)
        if len(x) <= MAX_LABELLED:
            for label, px, py in zip(labels, x.tolist(), y.tolist()):
                ax.annotate(str(label), (px, py), xytext=(3, 3), textcoords="offset points", fontsize=7)
        ax.axhline(0.0, color="0.8", linewidth=0.8, zorder=0)
        ax.axvline(0.0, color="0.8", linewidth=0.8, zorder=0)
        ax.set_xlabel(axis_label(result, 0))
        ax.set_ylabel(axis_label(result, 1) if two else "")
        ax.set_title(f"{name} principal coordinates")
        figure.tight_layout()
    except BaseException:
        plt.close(figure)
        raise
    return figure


def draw_ordination(result: ordination.Ordination, labels, name: str, filename: Path) -> None:
    """``ordination_figure`` saved as ``filename``."""
    figure = ordination_figure(result, labels, name)
    try:
        figure.savefig(filename)
    finally:
        import matplotlib.pyplot as plt

        plt.close(figure)
