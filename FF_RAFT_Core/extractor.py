from focusflow_official_amd.cce import BasicEncoder, ResidualBlock  # noqa: F401
