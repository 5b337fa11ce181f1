"""FedMLDefender singleton (reference: python/fedml/core/security/fedml_defender.py:40-196) for the
robust aggregators of this engine: krum / multikrum, trimmed_mean, wise_median,
coordinate_trimmed_mean (the per-coordinate trimmed mean of Yin et al. 2018, which the reference
lacks: its trimmed_mean trims whole clients and keeps that meaning here) and geometric_median (the
sample-weighted geometric median by the smoothed Weiszfeld iteration of Pillutla et al.; config
geomed_iters, geomed_nu; the reference's own RFA name stays unserved) and centered_clipping (centered
clipping of Karimireddy et al. around the global model or the mean, one iteration of which is
norm-difference clipping followed by FedAvg; config cclip_tau, cclip_iters, cclip_center; the
reference's cclip and norm_diff_clipping names stay unserved) and bulyan (El Mhamdi et al. 2018: Krum
repeated over one distance matrix, then per coordinate the mean of the values nearest the median over
the chosen clients; config byzantine_client_num; the contract is the paper's as written in
fedagg_robust.h and is not pinned to a reference fixture) and robust_lr (the robust learning rate of
Ozdayi et al. 2021 against backdoors: per coordinate the clients' updates vote with their signs and
the server's learning rate is negated where fewer than robust_lr_threshold net votes agree; config
robust_lr_threshold (required), robust_lr_server_lr, robust_lr_center; the reference's own
robust_learning_rate name stays unserved) and fools_gold (FoolsGold of Fung et al. 2018 against sybils:
before aggregation, every client's update is added into a running history and clients whose histories
point the same way are down-weighted or dropped; config fools_gold_use_memory, fools_gold_confidence,
fools_gold_center; the reference's own foolsgold name stays unserved).  Same dispatch
(which defenses act before / on / after aggregation) and the same entry points; the per-element work
runs in the HIP kernels (fedml_amd/csrc/median.hip, trimmed.hip, wsum_dist.hip, signvote.hip, pairdot.hip, robust.hip).  Other
defense types of the reference are outside the aggregation path and raise NotImplementedError when
configured.
"""
from __future__ import annotations

import logging
from collections import OrderedDict
from typing import Any, Callable, List, Tuple

from .constants import (DEFENSE_BULYAN, DEFENSE_CENTERED_CLIPPING, DEFENSE_COORD_TRIMMED_MEAN,
                        DEFENSE_FOOLS_GOLD, DEFENSE_GEOMETRIC_MEDIAN, DEFENSE_KRUM, DEFENSE_MULTIKRUM, DEFENSE_ROBUST_LR,
                        DEFENSE_TRIMMED_MEAN, DEFENSE_WISE_MEDIAN)
from .defense.bulyan_defense import BulyanDefense
from .defense.centered_clipping_defense import CenteredClippingDefense
from .defense.coordinate_trimmed_mean_defense import CoordinateTrimmedMeanDefense
from .defense.coordinate_wise_median_defense import CoordinateWiseMedianDefense
from .defense.coordinate_wise_trimmed_mean_defense import CoordinateWiseTrimmedMeanDefense
from .defense.fools_gold_defense import FoolsGoldDefense
from .defense.geometric_median_defense import GeometricMedianDefense
from .defense.krum_defense import KrumDefense
from .defense.robust_lr_defense import RobustLearningRateDefense


class FedMLDefender:
    _defender_instance = None

    @staticmethod
    def get_instance():
        if FedMLDefender._defender_instance is None:
            FedMLDefender._defender_instance = FedMLDefender()
        return FedMLDefender._defender_instance

    def __init__(self):
        self.is_enabled = False
        self.defense_type = None
        self.defender = None

    def init(self, args):
        if hasattr(args, "enable_defense") and args.enable_defense:
            self.args = args
            logging.info("------init defense..." + args.defense_type)
            self.is_enabled = True
            self.defense_type = args.defense_type.strip()
            if self.defense_type in (DEFENSE_KRUM, DEFENSE_MULTIKRUM):
                self.defender = KrumDefense(args)
            elif self.defense_type == DEFENSE_WISE_MEDIAN:
                self.defender = CoordinateWiseMedianDefense(args)
            elif self.defense_type == DEFENSE_TRIMMED_MEAN:
                self.defender = CoordinateWiseTrimmedMeanDefense(args)
            elif self.defense_type == DEFENSE_COORD_TRIMMED_MEAN:
                self.defender = CoordinateTrimmedMeanDefense(args)
            elif self.defense_type == DEFENSE_GEOMETRIC_MEDIAN:
                self.defender = GeometricMedianDefense(args)
            elif self.defense_type == DEFENSE_CENTERED_CLIPPING:
                self.defender = CenteredClippingDefense(args)
            elif self.defense_type == DEFENSE_BULYAN:
                self.defender = BulyanDefense(args)
            elif self.defense_type == DEFENSE_ROBUST_LR:
                self.defender = RobustLearningRateDefense(args)
            elif self.defense_type == DEFENSE_FOOLS_GOLD:
                self.defender = FoolsGoldDefense(args)
            else:
                raise NotImplementedError(
                    f"defense_type {self.defense_type!r} is not served by the MI355X engine "
                    f"(supported: krum, multikrum, trimmed_mean, wise_median, coordinate_trimmed_mean, "
                    f"geometric_median, centered_clipping, bulyan, robust_lr, fools_gold)")
        else:
            self.is_enabled = False
            self.defense_type = None
            self.defender = None

    def is_defense_enabled(self):
        return self.is_enabled

    def is_defense_on_aggregation(self):
        return self.is_defense_enabled() and self.defense_type in [DEFENSE_WISE_MEDIAN,
                                                                               DEFENSE_COORD_TRIMMED_MEAN,
                                                                               DEFENSE_GEOMETRIC_MEDIAN,
                                                                               DEFENSE_CENTERED_CLIPPING,
                                                                               DEFENSE_BULYAN,
                                                                               DEFENSE_ROBUST_LR]

    def is_defense_before_aggregation(self):
        return self.is_defense_enabled() and self.defense_type in [DEFENSE_KRUM, DEFENSE_MULTIKRUM,
                                                                   DEFENSE_TRIMMED_MEAN, DEFENSE_FOOLS_GOLD]

    def is_defense_after_aggregation(self):
        return False

    def defend_before_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                                  extra_auxiliary_info: Any = None):
        if self.defender is None:
            raise Exception("defender is not initialized!")
        if self.is_defense_before_aggregation():
            return self.defender.defend_before_aggregation(raw_client_grad_list, extra_auxiliary_info)
        return raw_client_grad_list

    def defend_on_aggregation(self, raw_client_grad_list: List[Tuple[float, OrderedDict]],
                              base_aggregation_func: Callable = None, extra_auxiliary_info: Any = None):
        if self.defender is None:
            raise Exception("defender is not initialized!")
        if self.is_defense_on_aggregation():
            return self.defender.defend_on_aggregation(raw_client_grad_list, base_aggregation_func,
                                                       extra_auxiliary_info)
        return base_aggregation_func(args=self.args, raw_grad_list=raw_client_grad_list)

    def defend_after_aggregation(self, global_model):
        if self.defender is None:
            raise Exception("defender is not initialized!")
        return global_model

    def get_malicious_client_idxs(self):
        return self.defender.get_malicious_client_idxs() if hasattr(self.defender, "get_malicious_client_idxs") else []

    def get_benign_client_idxs(self, client_idxs):
        return [i for i in client_idxs if i not in self.get_malicious_client_idxs()]
