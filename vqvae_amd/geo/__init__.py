"""Geometric analysis and graph-based utilities on the MI355X -- drop-in for the reference's
`src.geo` package (src/geo/__init__.py:5-8 re-exports the same two names), plus the K sweep of the
k-medoids analysis (fit_kmedoids_path, an extension), the matrix-free k-medoids refinement (fit_kmedoids_voronoi_graph,
cell_medoid_update_device, an extension) and the Riemannian graph experiments of the reference's
experiments/geo scripts (vqvae_amd.geo.experiments)."""
from .knn_graph_optimized import build_knn_graph, kneighbors, knn_query_device
from .geo_shortest_paths import dijkstra_multi_source
from .kmeans_optimized import cell_medoid_update_device, fit_kmedoids_path, fit_kmedoids_voronoi_graph
from .experiments import (mean_shortest_path, mean_shortest_path_device, pick_sources_from_lcc, reweight_edges_symmetric_device,
                          riemann_graph_effects, riemann_sanity, stratified_edge_sample)

__all__ = ["build_knn_graph", "cell_medoid_update_device", "dijkstra_multi_source", "fit_kmedoids_path", "fit_kmedoids_voronoi_graph",
           "kneighbors", "knn_query_device", "mean_shortest_path",
           "mean_shortest_path_device", "pick_sources_from_lcc", "reweight_edges_symmetric_device", "riemann_graph_effects", "riemann_sanity",
           "stratified_edge_sample"]
