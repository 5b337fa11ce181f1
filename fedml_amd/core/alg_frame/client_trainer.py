"""ClientTrainer plugin surface (reference: python/fedml/core/alg_frame/client_trainer.py:7-62).

The trainer-side counterpart of ServerAggregator: a client produces ``(num_samples, state_dict)``
-- the exact input format of the aggregation engine (``get_model_params`` returns a state_dict,
cf. ml/trainer/my_model_trainer_classification.py:15-16 in the reference).  Local DP
(``dp_solution_type="ldp"``, fedml_amd/core/dp) adds the client's noise to its parameters after local
training, on the HIP engine; the data poisoning hooks (core/security) are outside this engine and stay
off.
"""
from __future__ import annotations

from abc import ABC, abstractmethod

from ..dp.fedml_differential_privacy import FedMLDifferentialPrivacy


class ClientTrainer(ABC):
    def __init__(self, model, args):
        self.model = model
        self.id = 0
        self.args = args
        self.local_train_dataset = None
        self.local_test_dataset = None
        self.local_sample_number = 0
        if getattr(args, "enable_attack", False):
            raise NotImplementedError("args.enable_attack=True is outside the MI355X aggregation engine")
        FedMLDifferentialPrivacy.get_instance().init(args)

    def set_id(self, trainer_id):
        self.id = trainer_id

    def is_main_process(self):
        return True

    def update_dataset(self, local_train_dataset, local_test_dataset, local_sample_number):
        self.local_train_dataset = local_train_dataset
        self.local_test_dataset = local_test_dataset
        self.local_sample_number = local_sample_number

    @abstractmethod
    def get_model_params(self):
        ...

    @abstractmethod
    def set_model_params(self, model_parameters):
        ...

    def on_before_local_training(self, train_data, device, args):
        pass

    @abstractmethod
    def train(self, train_data, device, args):
        ...

    def on_after_local_training(self, train_data, device, args):
        """Reference :50-56: under local DP the client's parameters get its noise (its seed is derived
        from ``self.id``)."""
        dp = FedMLDifferentialPrivacy.get_instance()
        if dp.is_local_dp_enabled():
            self.set_model_params(dp.add_local_noise(self.get_model_params(), client_id=self.id))

    def test(self, test_data, device, args):
        pass
