"""Defense type names (reference: python/fedml/core/security/constants.py:1-19, the subset served here)."""
DEFENSE_KRUM = "krum"
DEFENSE_MULTIKRUM = "multikrum"
DEFENSE_TRIMMED_MEAN = "trimmed_mean"
DEFENSE_WISE_MEDIAN = "wise_median"
DEFENSE_COORD_TRIMMED_MEAN = "coordinate_trimmed_mean"  # no reference name: the per-coordinate trimmed mean (Yin et al. 2018)
DEFENSE_GEOMETRIC_MEDIAN = "geometric_median"  # no reference name here (its RFA stays unserved): smoothed Weiszfeld, contract in fedagg_robust.h
DEFENSE_CENTERED_CLIPPING = "centered_clipping"  # no reference name here (its cclip and norm_diff_clipping stay unserved): contract in fedagg_robust.h
DEFENSE_BULYAN = "bulyan"  # no reference fixture: the contract is the paper's (El Mhamdi et al. 2018) as written in fedagg_robust.h
DEFENSE_ROBUST_LR = "robust_lr"  # no reference name here (its robust_learning_rate stays unserved): the sign-vote learning rate of Ozdayi et al. 2021, contract in fedagg_robust.h
DEFENSE_FOOLS_GOLD = "fools_gold"  # no reference name here (its foolsgold stays unserved): the sybil defense of Fung et al. 2018 on the history Gram matrix, contract in fedagg_robust.h (fa_pairwise_dot)
