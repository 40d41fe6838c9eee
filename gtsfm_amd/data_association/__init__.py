"""Data association (gtsfm/data_association/): 2D feature tracks from the view graph's verified correspondences."""
