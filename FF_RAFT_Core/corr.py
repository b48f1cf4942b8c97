from focusflow_official_amd.corr_block import AlternateCorrBlock, CorrBlock  # noqa: F401
