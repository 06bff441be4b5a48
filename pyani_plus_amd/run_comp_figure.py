"""The two figures of plot-run-comp, drawn with matplotlib alone on the reference's grid
(pyani_plus/plot_run.py:422-493): the histogram of the reference run's identities above each column, one panel per
other run with the scatter (or the difference) and its red line, and the histogram of the panel's y values to its
right.  The histograms are drawn from the counts and edges ``run_comp`` computed (``Axes.stairs``), never from the
values.  matplotlib is imported when the first figure is drawn."""

from __future__ import annotations

from math import ceil, sqrt
from pathlib import Path

from . import run_comp


def grid_shape(n_others: int, columns: int = 0) -> tuple[int, int]:
    """``(plots_per_row, plots_per_col)``: ``columns`` panels a row, or a square tiling for 0."""
    per_row = columns if columns > 0 else ceil(sqrt(n_others))
    return per_row, ceil(n_others / per_row)


def comparison_figure(mode: str, ref_name: str, other_names: list[str], comparisons: list, columns: int = 0):
    """The figure of ``mode`` ``"scatter"`` (y against x, red diagonal) or ``"diff"`` (y - x against x, red zero line) for
    ``comparisons`` (``run_comp.Comparison``, one per other run); the caller closes it.  The histogram axes carry the
    labels ``hist_x_<column>`` and ``hist_y_<panel>``."""
    import matplotlib as mpl

    mpl.use("agg")  # non-interactive backend
    import matplotlib.pyplot as plt

    n = len(comparisons)
    per_row, per_col = grid_shape(n, columns)
    figure = plt.figure(figsize=(7 * per_row - 1, 1 + 5 * per_col))
    try:
        # (plot, hist-y), (spacer, plot, hist-y), ...; the x histograms in a thin first row
        grid = figure.add_gridspec(
            1 + per_col, 3 * per_row - 1, width_ratios=(5, 1) + (1, 5, 1) * (per_row - 1), height_ratios=(1,) + (5,) * per_col,
            left=0.15 / per_row, right=1 - 0.15 / per_row, bottom=0.15 / per_col, top=1 - 0.05 / per_col, wspace=0.05, hspace=0.05,
        )  # fmt: skip
        panels = [figure.add_subplot(grid[1, 0])]
        for k in range(1, n):
            panels.append(figure.add_subplot(grid[1 + k // per_row, 3 * (k % per_row)], sharex=panels[0], sharey=panels[0] if mode == "scatter" else None))
        for column in range(min(n, per_row)):
            ax_x = figure.add_subplot(grid[0, 3 * column], sharex=panels[0], label=f"hist_x_{column}")
            ax_x.spines[["left", "top", "right"]].set_visible(False)
            ax_x.get_yaxis().set_visible(False)
            ax_x.tick_params(axis="x", labelbottom=False)
            first = comparisons[0]
            if first.x_range is not None:
                ax_x.stairs(first.x_counts, run_comp.hist_edges(*first.x_range, len(first.x_counts)), fill=True)
        for k, (ax, comp) in enumerate(zip(panels, comparisons)):
            ax_y = figure.add_subplot(grid[1 + k // per_row, 1 + 3 * (k % per_row)], sharey=ax, label=f"hist_y_{k}")
            ax_y.tick_params(axis="y", labelleft=False)
            ax_y.get_xaxis().set_visible(False)
            ax_y.spines[["top", "right", "bottom"]].set_visible(False)
            if k // per_row + 1 == per_col:
                ax.set_xlabel(ref_name)
            else:
                ax.tick_params(axis="x", labelbottom=False)
            ax.spines[["top", "right"]].set_visible(False)
            x_lo, x_hi = float(comp.x.min()), float(comp.x.max())
            if mode == "diff":
                values, value_range, counts = comp.d, comp.d_range, comp.d_counts
                ax.plot([x_lo, x_hi], [0, 0], "-", color="r")
            else:
                values, value_range, counts = comp.y, comp.y_range, comp.y_counts
                ends = [max(x_lo, float(comp.y.min())), min(x_hi, float(comp.y.max()))]
                ax.plot(ends, ends, "-", color="r")
            ax.scatter(x=comp.x, y=values, s=2, alpha=0.2)
            ax.set_ylabel(other_names[k])
            ax_y.stairs(counts, run_comp.hist_edges(*value_range, len(counts)), orientation="horizontal", fill=True)
    except BaseException:
        plt.close(figure)
        raise
    return figure


def draw_comparison(mode: str, ref_name: str, other_names: list[str], comparisons: list, filename: Path, columns: int = 0) -> None:
    """``comparison_figure`` saved as ``filename``."""
    figure = comparison_figure(mode, ref_name, other_names, comparisons, columns)
    try:
        figure.savefig(filename)
    finally:
        import matplotlib.pyplot as plt

        plt.close(figure)
