"""Bundle adjustment (gtsfm/bundle/): all cameras and landmarks refined together on the MI355X."""
