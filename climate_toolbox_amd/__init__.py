"""MI355X-native weighted grid->region aggregation engine: a drop-in for the aggregation path of
ClimateImpactLab/climate_toolbox (``climate_toolbox.aggregations``).  See DESIGN.md."""

__version__ = "0.18.0"

from .aggregations import (  # noqa: F401
    weighted_aggregate_grid_to_regions,
    prepare_spatial_weights_data,
    prepare_weights,
    PreparedWeights,
    clear_caches,
    results_on_device,
    _reindex_spatial_data_to_regions,
    _aggregate_reindexed_data_to_regions,
)
from .many import weighted_aggregate_grid_to_regions_many  # noqa: F401  (several weightings / levels, one pass)
from .periods import weighted_aggregate_grid_to_regions_periods  # noqa: F401  (annual / monthly / labelled totals on the device)
from .seasons import (  # noqa: F401  (the reference's growing-season mask as per-cell day windows, summed on the device)
    season_boundaries,
    season_windows,
    get_daily_growing_season_mask,
    SeasonMask,
    SeasonWindows,
    day_of_year,
)
from .standardize import (  # noqa: F401  (coordinate standardisation folded into the plan)
    standardize_climate_data,
    convert_lons_split,
    convert_lons_mono,
    rename_coords_to_lon_and_lat,
)
from .relative import CellThresholds, cell_quantiles, cell_spell_reduce  # noqa: F401  (per-cell thresholds kept on the device)
from .transformations import (  # noqa: F401  (tas_poly fused into the aggregation)
    tas_poly,
    tas_poly_aggregate,
    snyder_edd,
    snyder_gdd,
    snyder_edd_aggregate,
    snyder_exposure_aggregate,
    tas_bins_aggregate,
    tas_hinge_aggregate,
    tas_rcspline_aggregate,
    tas_spell_aggregate,
    tas_rolling_aggregate,
    tas_quantile_aggregate,
    tas_relative_spell_aggregate,
    validate_edd_snyder_agriculture,
)
