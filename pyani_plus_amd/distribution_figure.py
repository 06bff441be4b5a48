"""The distribution figure of plot-run, drawn with matplotlib alone in the reference's layout
(pyani_plus/plot_run.py:153-215): 15 x 5 in, the histogram of the score on the left, its kernel density on the right
with a rug under the axis, the reference's x-limits per score.  Everything is drawn from what ``distribution``
computed -- counts and edges (``Axes.stairs``), the density on its grid, the rug's counts per pixel column (one
``LineCollection``, a column's opacity ``1 - 0.9 ** count``: what that many lines of alpha 0.1 on top of each other
come to) -- never from the values.  matplotlib is imported when the first figure is drawn."""

from __future__ import annotations

from pathlib import Path

import numpy as np

from . import distribution

FILL = "#A6C8E0"
RUG = "#2678B2"
RUG_HEIGHT = -0.025  # of the axes' height: below the axis, as in the reference


def distribution_figure(dist: distribution.Distribution, rug: tuple[np.ndarray, np.ndarray], name: str):
    """The figure of score ``name``; the caller closes it.  ``rug``: ``distribution.rug_counts``."""
    import matplotlib as mpl

    mpl.use("agg")  # non-interactive backend
    import matplotlib.pyplot as plt
    from matplotlib.collections import LineCollection
    from matplotlib.colors import to_rgb

    figure, axes = plt.subplots(1, 2, figsize=(15, 5))
    try:
        figure.suptitle(f"{name} distribution")
        axes[0].stairs(dist.counts, dist.edges, fill=True, color=FILL)
        axes[0].set_ylabel("Count")
        axes[0].set_ylim(bottom=0)
        if dist.grid is not None:
            axes[1].plot(dist.grid, dist.density)
        axes[1].set_ylabel("Density")
        axes[1].set_ylim(bottom=0)
        if name in distribution.X_LIMITS:
            for ax in axes:
                ax.set_xlim(*distribution.X_LIMITS[name])
        rug_edges, rug_counts = rug
        seen = rug_counts > 0
        centres = ((rug_edges[:-1] + rug_edges[1:]) / 2)[seen]
        colours = np.empty((len(centres), 4))
        colours[:, :3] = to_rgb(RUG)
        colours[:, 3] = 1.0 - np.power(0.9, rug_counts[seen].astype(np.float64))
        lines = LineCollection([((x, 0.0), (x, RUG_HEIGHT)) for x in centres.tolist()], colors=colours, linewidths=1.0,
                               transform=axes[1].get_xaxis_transform(), clip_on=False, label="rug")  # fmt: skip
        axes[1].add_collection(lines, autolim=False)
        figure.tight_layout(rect=(0, 0.03, 1, 0.95))
    except BaseException:
        plt.close(figure)
        raise
    return figure


def draw_distribution(dist: distribution.Distribution, rug: tuple[np.ndarray, np.ndarray], name: str, filename: Path) -> None:
    """``distribution_figure`` saved as ``filename``."""
    figure = distribution_figure(dist, rug, name)
    try:
        figure.savefig(filename)
    finally:
        import matplotlib.pyplot as plt

        plt.close(figure)
