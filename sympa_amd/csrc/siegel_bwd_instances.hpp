// The Siegel backward kernel instances that get a compile job of their own, one per line.  This is the ONLY list of them:
//   * the build (__graft_entry__.hip_units) reads the lines with a regular expression and compiles the family's instance
//     source once per line with -DSYMPA_INST_MODEL / _N / _FORM set to the line's words: one object, one DPP hazard scan
//     and, where the scan fails, one rebuild in the safe form per KERNEL, and the fully unrolled n = 7, 8 adjoints (minutes
//     each) compile in parallel;
//   * the headers declare each line's wrapper function and the dispatch units test each line in turn, by including this
//     file with the family's macro defined.
// A new instance is a new line.  Keep the lines flat (no helper macros, one instance per line, ", " between the words):
// the build does not run the preprocessor.  Macros left undefined by the includer expand to nothing; all are undefined
// at the end, so the file can be included again.  (No include guard for that reason.)
//
//   family (instance source, wrapper)                                    words
//   SYMPA_BWD_COOP            siegel_bwd_coop_instance.hip               model, n = 9..16, output form
//                             launch_bwd_coop_<model>_<n>_<form>         sixteen lanes per pair
//   SYMPA_BWD_HALF            siegel_bwd_half_instance.hip               model, n = 5..8, output form
//                             launch_bwd_half_<model>_<n>_<form>         eight lanes per pair
//   SYMPA_BWD_SPLIT_SPECTRAL  siegel_bwd_split_instance.hip              model, n = 5..8 (stage 1 writes the workspace only)
//                             launch_bwd_split_spectral_<model>_<n>
//   SYMPA_BWD_SPLIT_GRADIENT  siegel_bwd_split_instance.hip              model, n = 5..8, output form
//                             launch_bwd_split_gradient_<model>_<n>_<form>
//   SYMPA_BWD_ONE_LANE        siegel_bwd_one_lane_instance.hip           model, n = 7, 8, output form
//                             launch_bwd_n<n>_<model>_<form>             one pair per lane (dims <= 6 share siegel_bwd.hip)
// model: upper | bounded | dual; output form: dense (per-pair gradient rows) | scatter (atomic adds into the table gradient).
#ifndef SYMPA_BWD_COOP
#define SYMPA_BWD_COOP(model, n, form)
#endif
#ifndef SYMPA_BWD_HALF
#define SYMPA_BWD_HALF(model, n, form)
#endif
#ifndef SYMPA_BWD_SPLIT_SPECTRAL
#define SYMPA_BWD_SPLIT_SPECTRAL(model, n)
#endif
#ifndef SYMPA_BWD_SPLIT_GRADIENT
#define SYMPA_BWD_SPLIT_GRADIENT(model, n, form)
#endif
#ifndef SYMPA_BWD_ONE_LANE
#define SYMPA_BWD_ONE_LANE(model, n, form)
#endif

SYMPA_BWD_COOP(upper, 9, dense)
SYMPA_BWD_COOP(upper, 9, scatter)
SYMPA_BWD_COOP(upper, 10, dense)
SYMPA_BWD_COOP(upper, 10, scatter)
SYMPA_BWD_COOP(upper, 11, dense)
SYMPA_BWD_COOP(upper, 11, scatter)
SYMPA_BWD_COOP(upper, 12, dense)
SYMPA_BWD_COOP(upper, 12, scatter)
SYMPA_BWD_COOP(upper, 13, dense)
SYMPA_BWD_COOP(upper, 13, scatter)
SYMPA_BWD_COOP(upper, 14, dense)
SYMPA_BWD_COOP(upper, 14, scatter)
SYMPA_BWD_COOP(upper, 15, dense)
SYMPA_BWD_COOP(upper, 15, scatter)
SYMPA_BWD_COOP(upper, 16, dense)
SYMPA_BWD_COOP(upper, 16, scatter)
SYMPA_BWD_COOP(bounded, 9, dense)
SYMPA_BWD_COOP(bounded, 9, scatter)
SYMPA_BWD_COOP(bounded, 10, dense)
SYMPA_BWD_COOP(bounded, 10, scatter)
SYMPA_BWD_COOP(bounded, 11, dense)
SYMPA_BWD_COOP(bounded, 11, scatter)
SYMPA_BWD_COOP(bounded, 12, dense)
SYMPA_BWD_COOP(bounded, 12, scatter)
SYMPA_BWD_COOP(bounded, 13, dense)
SYMPA_BWD_COOP(bounded, 13, scatter)
SYMPA_BWD_COOP(bounded, 14, dense)
SYMPA_BWD_COOP(bounded, 14, scatter)
SYMPA_BWD_COOP(bounded, 15, dense)
SYMPA_BWD_COOP(bounded, 15, scatter)
SYMPA_BWD_COOP(bounded, 16, dense)
SYMPA_BWD_COOP(bounded, 16, scatter)

SYMPA_BWD_HALF(upper, 5, dense)
SYMPA_BWD_HALF(upper, 5, scatter)
SYMPA_BWD_HALF(upper, 6, dense)
SYMPA_BWD_HALF(upper, 6, scatter)
SYMPA_BWD_HALF(upper, 7, dense)
SYMPA_BWD_HALF(upper, 7, scatter)
SYMPA_BWD_HALF(upper, 8, dense)
SYMPA_BWD_HALF(upper, 8, scatter)
SYMPA_BWD_HALF(bounded, 5, dense)
SYMPA_BWD_HALF(bounded, 5, scatter)
SYMPA_BWD_HALF(bounded, 6, dense)
SYMPA_BWD_HALF(bounded, 6, scatter)
SYMPA_BWD_HALF(bounded, 7, dense)
SYMPA_BWD_HALF(bounded, 7, scatter)
SYMPA_BWD_HALF(bounded, 8, dense)
SYMPA_BWD_HALF(bounded, 8, scatter)

SYMPA_BWD_SPLIT_SPECTRAL(upper, 5)
SYMPA_BWD_SPLIT_SPECTRAL(upper, 6)
SYMPA_BWD_SPLIT_SPECTRAL(upper, 7)
SYMPA_BWD_SPLIT_SPECTRAL(upper, 8)
SYMPA_BWD_SPLIT_SPECTRAL(bounded, 5)
SYMPA_BWD_SPLIT_SPECTRAL(bounded, 6)
SYMPA_BWD_SPLIT_SPECTRAL(bounded, 7)
SYMPA_BWD_SPLIT_SPECTRAL(bounded, 8)

SYMPA_BWD_SPLIT_GRADIENT(upper, 5, dense)
SYMPA_BWD_SPLIT_GRADIENT(upper, 5, scatter)
SYMPA_BWD_SPLIT_GRADIENT(upper, 6, dense)
SYMPA_BWD_SPLIT_GRADIENT(upper, 6, scatter)
SYMPA_BWD_SPLIT_GRADIENT(upper, 7, dense)
SYMPA_BWD_SPLIT_GRADIENT(upper, 7, scatter)
SYMPA_BWD_SPLIT_GRADIENT(upper, 8, dense)
SYMPA_BWD_SPLIT_GRADIENT(upper, 8, scatter)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 5, dense)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 5, scatter)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 6, dense)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 6, scatter)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 7, dense)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 7, scatter)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 8, dense)
SYMPA_BWD_SPLIT_GRADIENT(bounded, 8, scatter)

SYMPA_BWD_ONE_LANE(upper, 7, dense)
SYMPA_BWD_ONE_LANE(upper, 7, scatter)
SYMPA_BWD_ONE_LANE(upper, 8, dense)
SYMPA_BWD_ONE_LANE(upper, 8, scatter)
SYMPA_BWD_ONE_LANE(bounded, 7, dense)
SYMPA_BWD_ONE_LANE(bounded, 7, scatter)
SYMPA_BWD_ONE_LANE(bounded, 8, dense)
SYMPA_BWD_ONE_LANE(bounded, 8, scatter)
SYMPA_BWD_ONE_LANE(dual, 7, dense)
SYMPA_BWD_ONE_LANE(dual, 7, scatter)
SYMPA_BWD_ONE_LANE(dual, 8, dense)
SYMPA_BWD_ONE_LANE(dual, 8, scatter)

#undef SYMPA_BWD_COOP
#undef SYMPA_BWD_HALF
#undef SYMPA_BWD_SPLIT_SPECTRAL
#undef SYMPA_BWD_SPLIT_GRADIENT
#undef SYMPA_BWD_ONE_LANE
