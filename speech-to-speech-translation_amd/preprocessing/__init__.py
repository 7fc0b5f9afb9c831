"""Data preparation stages of ``examples/s2s_trans/run_baseline.sh`` that run in this package (stage 3: features)."""
