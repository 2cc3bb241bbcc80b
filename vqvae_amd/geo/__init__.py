"""Geometric analysis and graph-based utilities on the MI355X -- drop-in for the reference's
`src.geo` package (src/geo/__init__.py:5-8 re-exports the same two names), plus the K sweep of the
k-medoids analysis (fit_kmedoids_path, an extension), the matrix-free k-medoids refinement (fit_kmedoids_voronoi_graph,
cell_medoid_update_device, an extension) and the Riemannian graph experiments of the reference's
experiments/geo scripts (vqvae_amd.geo.experiments), and the bridging of a kNN graph's components (bridge_components_device,
nearest_foreign_device, connect_components, an extension), and the pull-back metric tensor per latent (pullback_metric,
pullback_metric_device, native_metric_covers, an extension), and geodesic paths and interpolation along them (geodesic_paths,
geodesic_paths_device, paths_from_predecessors_device, resample_paths_device, chord_frames_device, geodesic_interpolation,
interpolate_images_spatial, interpolate_images_vanilla, an extension), and the relaxation of curves under the pull-back metric (curve_energy_device,
relax_curves_device, native_relax_covers, an extension), and the same under the vanilla decoder through its vector-Jacobian
product (native_vanilla_relax_covers, vanilla_vjp_device, an extension), and image curves under the whole spatial decoder on 4x4
grids (native_grid_relax_covers, spatial_grid_vjp_device, grid_curve_energy_device, relax_grid_curves_device, an extension), and
the metric tensor of the vanilla decoder with a batched symmetric eigenvalue kernel (native_vanilla_metric_covers,
sym_spectrum_device, an extension)."""
from .knn_graph_optimized import (bridge_components_device, build_knn_graph, connect_components, kneighbors, knn_query_device,
                                  nearest_foreign_device)
from .geo_shortest_paths import (GeodesicPaths, chord_frames_device, dijkstra_multi_source, geodesic_paths, geodesic_paths_device,
                                 paths_from_predecessors_device, resample_paths_device)
from .interpolation import geodesic_interpolation, interpolate_images_spatial, interpolate_images_vanilla
from .kmeans_optimized import cell_medoid_update_device, fit_kmedoids_path, fit_kmedoids_voronoi_graph
from .experiments import (mean_shortest_path, mean_shortest_path_device, pick_sources_from_lcc, reweight_edges_symmetric_device,
                          riemann_graph_effects, riemann_sanity, stratified_edge_sample)
from .riemannian_metric import (PullbackMetric, native_metric_covers, native_vanilla_metric_covers, pullback_metric,
                                pullback_metric_device, sym_spectrum_device, vanilla_vjp_device)
from .relaxation import (CurveEnergy, RelaxedCurves, curve_energy_device, native_relax_covers, native_vanilla_relax_covers,
                         relax_curves_device)
from .grid_relaxation import (grid_curve_energy_device, native_grid_relax_covers, relax_grid_curves_device,
                              spatial_grid_vjp_device)

__all__ = ["bridge_components_device", "build_knn_graph", "cell_medoid_update_device", "connect_components", "dijkstra_multi_source", "fit_kmedoids_path", "fit_kmedoids_voronoi_graph",
           "kneighbors", "knn_query_device", "mean_shortest_path",
           "PullbackMetric", "native_metric_covers", "native_vanilla_metric_covers", "pullback_metric", "pullback_metric_device",
           "sym_spectrum_device",
           "mean_shortest_path_device", "nearest_foreign_device", "pick_sources_from_lcc", "reweight_edges_symmetric_device", "riemann_graph_effects", "riemann_sanity",
           "stratified_edge_sample",
           "GeodesicPaths", "chord_frames_device", "geodesic_paths", "geodesic_paths_device", "paths_from_predecessors_device",
           "resample_paths_device", "geodesic_interpolation", "interpolate_images_spatial", "interpolate_images_vanilla",
           "CurveEnergy", "RelaxedCurves", "curve_energy_device", "native_relax_covers", "native_vanilla_relax_covers",
           "relax_curves_device", "vanilla_vjp_device",
           "grid_curve_energy_device", "native_grid_relax_covers", "relax_grid_curves_device", "spatial_grid_vjp_device"]
