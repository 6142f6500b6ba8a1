// hc_morison_members.hpp -- what hc_morison.hip (the lane's begin / end) needs of the strip members (hc_morison_members.hip).
#pragma once

struct hc_ctx;

namespace hc {

// members on the bodies this context owns
int members_owned(const hc_ctx* c);
// The member launches of one evaluation, on the Morison lane's stream behind whatever it holds: the lane's component table
// (c->mor.kin) is current and `d_state` ([12 N] pos | rpy | linvel | angvel) is on its way on the same stream.  `order2`: the
// members see the second-order sea in this evaluation -- the lane's pair tables (c->mor2: Order2Part::prepare has answered true) are
// current too, and the increments of the nodes and the Gauss points go to the host copy in flight (c->members.copies).
void members_enqueue(hc_ctx* c, double t, const double* d_state, bool order2);

}  // namespace hc
