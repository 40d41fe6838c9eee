"""View-graph estimators (gtsfm/view_graph_estimator/): which two-view edges reach rotation averaging."""
