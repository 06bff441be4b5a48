"""The scatter figure of plot-run, drawn with matplotlib alone in the layout ``seaborn.jointplot`` gives the reference
(pyani_plus/plot_run.py:218-299): 6 x 6 in, a joint panel with a margin above and one to the right (a grid of ratio 5
with space 0.2), the reference's ``subplots_adjust(left=0.2, right=0.8, top=0.8, bottom=0.2)`` and its colour bar at
``[0.85, 0.25, 0.05, 0.4]``.  Everything is drawn from what ``scatter.describe`` computed -- the joint panel is the
colour grid as one image over the cell edges (viridis between the smallest and the largest query length), the margins
are the two automatic histograms (``Axes.stairs``, the y one horizontal) -- never from the values.  matplotlib is
imported when the first figure is drawn."""

from __future__ import annotations

from pathlib import Path

import numpy as np

from . import scatter

RATIO = 5  # jointplot's: the joint panel's share of the grid against a margin's 1
SPACE = 0.2  # jointplot's: the gap between the panels
FILL = "#A6C8E0"
X_LABEL = "Percent identity (ANI)"
BAR_LABEL = "Query length (bp)"


def scatter_figure(data: scatter.Scatter, caption: str):
    """The figure of identity against the score with axis label ``caption``; the caller closes it.  Its axes are
    labelled ``joint``, ``x margin``, ``y margin`` and ``colour bar``."""
    import matplotlib as mpl

    mpl.use("agg")  # non-interactive backend
    import matplotlib.pyplot as plt
    from matplotlib.colors import Normalize

    figure = plt.figure(figsize=(6, 6))
    try:
        grid = figure.add_gridspec(RATIO + 1, RATIO + 1, hspace=SPACE, wspace=SPACE)
        joint = figure.add_subplot(grid[1:, :-1], label="joint")
        top = figure.add_subplot(grid[0, :-1], sharex=joint, label="x margin")
        right = figure.add_subplot(grid[1:, -1], sharey=joint, label="y margin")
        # pcolormesh takes rows = y: the grid is x first
        mesh = joint.pcolormesh(data.xedges, data.yedges, np.ma.masked_invalid(data.colour.T), cmap="viridis",
                                norm=Normalize(data.c_min, data.c_max), shading="flat", rasterized=True)  # fmt: skip
        joint.set_xlabel(X_LABEL)
        joint.set_ylabel(caption)
        top.stairs(data.x_hist.counts, data.x_hist.edges, fill=True, color=FILL)
        right.stairs(data.y_hist.counts, data.y_hist.edges, fill=True, color=FILL, orientation="horizontal")
        top.set_ylim(bottom=0)
        right.set_xlim(left=0)
        for ax in (top, right):  # jointplot hides the margins' own ticks and labels
            ax.tick_params(labelbottom=ax is right, labelleft=ax is top)
            for side in ("top", "right"):
                ax.spines[side].set_visible(False)
        top.tick_params(labelleft=False)
        right.tick_params(labelbottom=False)
        figure.subplots_adjust(left=0.2, right=0.8, top=0.8, bottom=0.2)
        bar = figure.colorbar(mesh, cax=figure.add_axes([0.85, 0.25, 0.05, 0.4], label="colour bar"))
        bar.set_label(BAR_LABEL)
    except BaseException:
        plt.close(figure)
        raise
    return figure


def draw_scatter(data: scatter.Scatter, caption: str, filename: Path) -> None:
    """``scatter_figure`` saved as ``filename``."""
    figure = scatter_figure(data, caption)
    try:
        figure.savefig(filename)
    finally:
        import matplotlib.pyplot as plt

        plt.close(figure)
