"""Top-level `data` package of the reference layout, re-exporting the MI355X-native mirrors."""
