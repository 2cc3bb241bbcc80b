"""Geometric analysis and graph-based utilities on the MI355X -- drop-in for the reference's
`src.geo` package (src/geo/__init__.py:5-8 re-exports the same two names), plus the K sweep of the
k-medoids analysis (fit_kmedoids_path, an extension)."""
from .knn_graph_optimized import build_knn_graph
from .geo_shortest_paths import dijkstra_multi_source
from .kmeans_optimized import fit_kmedoids_path

__all__ = ["build_knn_graph", "dijkstra_multi_source", "fit_kmedoids_path"]
