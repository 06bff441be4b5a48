"""The heatmap figure of plot-run, drawn with matplotlib alone (the reference draws it with seaborn's ``clustermap``,
pyani_plus/plot_run.py:75-150): the reordered matrix with the reference's colour maps and limits, NaN cells in its
orange, and the row dendrogram built from the linkage table.  matplotlib is imported when the first figure is drawn."""

from __future__ import annotations

from pathlib import Path

import numpy as np

ORANGE = (0.934, 0.422, 0)
GREY = (0.7, 0.7, 0.7)
DULL_BLUE = (0.137, 0.412, 0.737)
WHITE = (1.0, 1.0, 1.0)
DULL_RED = (0.659, 0.216, 0.231)
MAX_FIGSIZE = 120


def colour_map(name: str):
    """``spbnd_BuRd`` (grey below 80 %, blue to white at the 95 % species boundary, red at 100 %), ``BuRd`` (blue, white,
    red) or one of matplotlib's own, with NaN cells in orange."""
    from matplotlib import colormaps
    from matplotlib.colors import LinearSegmentedColormap

    if name == "spbnd_BuRd":
        cmap = LinearSegmentedColormap.from_list(name, ((0.00, GREY), (0.80, GREY), (0.80, DULL_BLUE), (0.95, WHITE), (1.00, DULL_RED)))
    elif name == "BuRd":
        cmap = LinearSegmentedColormap.from_list(name, ((0.0, DULL_BLUE), (0.5, WHITE), (1.0, DULL_RED)))
    else:
        cmap = colormaps[name]
    return cmap.with_extremes(bad=ORANGE)


def dendrogram_segments(tree: np.ndarray, leaves) -> list[tuple[tuple[float, float, float, float], tuple[float, float, float, float]]]:
    """The U-shaped links of the dendrogram of ``tree`` (scipy's linkage table) as (heights, positions) of their four
    corners; leaf ``leaves[k]`` sits at position ``k + 0.5``, a cluster midway between its two sides."""
    n = len(leaves)
    position = np.zeros(2 * n - 1)
    height = np.zeros(2 * n - 1)
    position[np.asarray(leaves, dtype=np.int64)] = np.arange(n) + 0.5
    links = []
    for r, (a, b, dist, _size) in enumerate(tree):
        a, b = int(a), int(b)
        position[n + r] = (position[a] + position[b]) / 2.0
        height[n + r] = dist
        links.append(((height[a], dist, dist, height[b]), (position[a], position[a], position[b], position[b])))
    return links


def draw_heatmap(table, tree: np.ndarray, leaves, name: str, color_scheme: str, filename: Path) -> None:
    """``table`` (a frame already in leaf order) as a heatmap with the row dendrogram of ``tree`` on its left; figure size
    ``min(max(8, 1.1 n), 120)`` inches, ``vmin`` 0, ``vmax`` 5 for tANI and 1 otherwise."""
    import matplotlib as mpl

    mpl.use("agg")  # non-interactive backend
    import matplotlib.pyplot as plt

    n = len(table)
    figsize = min(max(8, n * 1.1), MAX_FIGSIZE)
    figure = plt.figure(figsize=(figsize, figsize))
    try:
        grid = figure.add_gridspec(2, 2, width_ratios=(0.2, 0.8), height_ratios=(0.2, 0.8), wspace=0.01, hspace=0.01)
        ax_heat = figure.add_subplot(grid[1, 1])
        ax_rows = figure.add_subplot(grid[1, 0])
        ax_bar = figure.add_subplot(grid[0, 0])
        values = np.ma.masked_invalid(table.to_numpy(dtype=float))
        mesh = ax_heat.pcolormesh(values, cmap=colour_map(color_scheme), vmin=0, vmax=5 if name == "tANI" else 1, edgecolors="white", linewidth=0.25)
        ax_heat.set_ylim(n, 0)  # first leaf at the top
        ticks = np.arange(n) + 0.5
        ax_heat.set_xticks(ticks, [str(x) for x in table.columns], rotation=90)
        ax_heat.set_yticks(ticks, [str(x) for x in table.index])
        ax_heat.yaxis.tick_right()
        for heights, positions in dendrogram_segments(tree, leaves):
            ax_rows.plot(heights, positions, color="0.2", linewidth=0.7)
        ax_rows.set_ylim(n, 0)
        ax_rows.invert_xaxis()  # the root on the left
        ax_rows.set_axis_off()
        bar_box = ax_bar.get_position()
        ax_bar.set_position((bar_box.xmin, bar_box.ymin, min(0.05, bar_box.width), bar_box.height))
        figure.colorbar(mesh, cax=ax_bar)
        figure.savefig(filename, bbox_inches="tight")
    finally:
        plt.close(figure)
