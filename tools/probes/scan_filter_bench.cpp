// scan_filter_bench.cpp -- the host's timer on the raw scan's filter alone: the ONE-loop form (what scan_filter_stage ran
// before csrc/scan_filter.cpp; kept verbatim in tests/native/scan_filter_test.cpp too) against the keep-mask pass +
// compaction pass, 1080 beams, 32 of them unoccupied, a fresh pose per call, the minimum of 2000 calls; on an
// unbounded map (the headline's scans: no geometry) and on a bounded one with tabulated beam trig.
//   hipcc -O3 -std=c++17 -ffp-contract=off -I slam-constructor_amd/csrc tools/probes/scan_filter_bench.cpp \
//         slam-constructor_amd/csrc/scan_filter.cpp -o scan_filter_bench
#include <chrono>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "scan_filter.h"
static double now(){return std::chrono::duration<double,std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();}
int main(){
  const int n=1080; std::vector<double> range(n),angle(n),ca(n),sa(n); std::vector<int> occ(n,1);
  for(int i=0;i<n;++i){range[i]=5+0.01*i; angle[i]=-2.35+i*0.00436; ca[i]=cos(angle[i]); sa[i]=sin(angle[i]); if(i%34==5) occ[i]=0;}
  for(int bounded=0;bounded<2;++bounded){
    std::vector<int> kept; kept.reserve(n); double best_old=1e9,best_new=1e9; long acc=0;
    for(int rep=0;rep<2000;++rep){
      double pose[3]={0.1+rep*1e-4,0.2,0.3+rep*1e-5};
      double t0=now();
      { constexpr double eps=std::numeric_limits<double>::epsilon(); double max_range=-1; unsigned skip_rate=0; const int*is_occ=occ.data();
        kept.clear(); const bool cut=0.0<max_range+eps; double sb=0,cb=1; if(bounded) ::sincos(pose[2],&sb,&cb);
        double scale=0.05; int ox=1000,oy=1000,w=2000,h=2000;
        for(int i=0;i<n;++i){ if(skip_rate&&(unsigned(i)%skip_rate))continue; if(is_occ&&!is_occ[i])continue; const bool too_far=cut&&(max_range<range[i]+eps); if(too_far)continue;
          if(bounded){double c=cb*ca[i]-sb*sa[i], s=sb*ca[i]+cb*sa[i]; const double wx=pose[0]+range[i]*c, wy=pose[1]+range[i]*s; const int ix=(int)std::floor(wx/scale)+ox, iy=(int)std::floor(wy/scale)+oy; if(!(0<=ix&&ix<w&&0<=iy&&iy<h))continue;}
          kept.push_back(i);} }
      double t1=now(); acc+=kept.size(); if(t1-t0<best_old)best_old=t1-t0;
      static std::vector<unsigned char> mask(n); static std::vector<int> k2(n);
      t0=now();
      slamhip::ScanFilterArgs a{}; a.n=n;a.range=range.data();a.angle=angle.data();a.is_occ=occ.data();a.max_range=-1;a.bounded=bounded;a.cos_a=ca.data();a.sin_a=sa.data();a.pose[0]=pose[0];a.pose[1]=pose[1];a.pose[2]=pose[2];a.scale=0.05;a.origin_x=a.origin_y=1000;a.width=a.height=2000;
      slamhip::scan_filter_mask(a,mask.data(),nullptr); int k=slamhip::scan_filter_compact(mask.data(),n,k2.data());
      t1=now(); acc+=k; if(t1-t0<best_new)best_new=t1-t0;
    }
    printf("bounded %d: old %.2f us, new %.2f us (min of 2000) %ld\n",bounded,best_old,best_new,acc);
  }
}
